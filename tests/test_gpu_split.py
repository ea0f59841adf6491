"""Every pass off the tile grid and at band heights other than 8 (tests/split_cases.py has the geometry and
tests/test_split_cases.py qualifies it on the CPU oracle): frames 203 x 77 and 124 x 45, whose partial edge
tiles hold hits, misses, lit and shadowed pixels, split in bands of 1, 3, 5, 8, 12 and 50 rows over 2 and 3
ranks, round-robin and by an owner cycle of 5, some of which own no row.

Every comparison is byte equality with the CPU oracle, or with the numpy models the suite already has where
the oracle has no such pass (tests/reflect_util.py, tests/ambient_util.py, sky.sample_sky,
tests/lod_tracer.py).  Every device buffer a call may write is followed by a pattern-filled guard of 4 KiB
that is checked afterwards (split_cases.Arena), so a small overrun fails an assertion."""
import ctypes

import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, RaytracingMaster, SVOData
from raytracingtest_amd import _lib
from raytracingtest_amd._lib import LAYOUT_BAND, LAYOUT_FRAME
from raytracingtest_amd.camera import jitter_offsets, main_light
from tests import split_cases as sc

pytestmark = pytest.mark.gpu

WEIGHTED_DEALS = (3, 5, 12)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def contexts(torch):
    """One context per svo_config, made on first use and kept for the module."""
    made = {}

    def get(**config):
        key = tuple(sorted(config.items()))
        if key not in made:
            m = RaytracingMaster(device=0, capacity_nodes=len(sc.pool()), config=config)
            m.SetSVOBuffer(sc.pool())
            made[key] = m
        return made[key]
    yield get
    for m in made.values():
        m.close()


def set_view(m, frame, camera=None):
    w, h = sc.FRAMES[frame]
    m.UpdateShaderParameters(sc.edge_camera() if camera is None else camera, w, h)
    return w, h


def same(got, want, item, what):
    """Byte equality of a device buffer's copy with the expected bytes, with a count on failure."""
    got = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    want = np.frombuffer(want if isinstance(want, bytes) else np.ascontiguousarray(want).tobytes(), np.uint8)
    assert len(got) == len(want), f"{what}: {len(got)} bytes, expected {len(want)}"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.reshape(-1, item) != want.reshape(-1, item)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got) // item} entries differ, first {bad[:8].tolist()}")


def item_of(key):
    return sc.ITEM.get(key, 8)


def check_band_layout(torch, m, frame, band, mode, ref, keys, what, launches=1):
    """Band-layout renders of `band` (None: the whole frame): every output in `keys` equals the expected
    frame's rows, guards untouched -- on each of `launches` launches in a row.  A rank without rows gets
    guard-only buffers, returns SVO_OK and writes nothing."""
    w, h = sc.FRAMES[frame]
    ys = sc.rows_of(h, band)
    arena = sc.Arena(torch, sc.band_sizes(w, h, band, keys))
    for launch in range(launches):
        if launch:
            arena.reset()
        m.render_frame(w, h, stack_mode=mode, band=band, layout=LAYOUT_BAND, **arena.ptrs(keys))
        m.synchronize()
        arena.fetch()
        for k in keys:
            same(arena.get(k), sc.expected_rows(ref, ys, k), item_of(k), f"{what} launch {launch}: {k}")
        arena.check_guards(f"{what} launch {launch}")
    return arena


def check_frame_layout(torch, m, frame, rows, split, mode, ref, keys, what, in_turn=False):
    """Every rank of a deal renders in place into one pattern-filled frame (frame layout; the hit masks are
    band-local, one buffer per rank).  After the last rank the frame is the expected one.  in_turn: checked
    after every rank -- its rows exact, the rows of the ranks still to come untouched."""
    w, h = sc.FRAMES[frame]
    pix = [k for k in keys if k != "hitmask"]
    sizes = {k: w * h * sc.ITEM[k] for k in pix}
    if "hitmask" in keys:
        for r in sc.ranks(split):
            sizes[f"hitmask{r}"] = sc.n_tiles(w, len(sc.rows_of(h, sc.band_of(rows, r, split)))) * 8
    arena = sc.Arena(torch, sizes)
    done = np.zeros(h, bool)
    last = max(sc.ranks(split))
    for r in sc.ranks(split):
        band = sc.band_of(rows, r, split)
        ptrs = arena.ptrs(pix)
        if "hitmask" in keys:
            ptrs["hitmask"] = arena.ptr(f"hitmask{r}")
        m.render_frame(w, h, stack_mode=mode, band=band, layout=LAYOUT_FRAME, **ptrs)
        done[sc.rows_of(h, band)] = True
        if not (in_turn or r == last):
            continue
        m.synchronize()
        arena.fetch()
        for k in pix:
            got = arena.get(k).reshape(h, w * sc.ITEM[k])
            want = np.ascontiguousarray(ref[k]).view(np.uint8).reshape(h, w * sc.ITEM[k])
            same(got[done], want[done], sc.ITEM[k], f"{what} frame layout after rank {r}: {k}")
            assert np.all(got[~done] == sc.FILL), f"{what} frame layout after rank {r}: {k} written outside the rank's rows"
        if "hitmask" in keys:
            for q in range(r + 1):
                ys = sc.rows_of(h, sc.band_of(rows, q, split))
                same(arena.get(f"hitmask{q}"), sc.expected_rows(ref, ys, "hitmask"), 8, f"{what} frame layout: hit mask of rank {q}")
            for q in range(r + 1, last + 1):
                assert arena.untouched(f"hitmask{q}")
        arena.check_guards(f"{what} frame layout after rank {r}")
    assert done.all()


def check_deal(torch, m, frame, rows, split, mode, ref, keys, what, launches=2):
    for r in sc.ranks(split):
        check_band_layout(torch, m, frame, sc.band_of(rows, r, split), mode, ref, keys, f"{what} rank {r}", launches)
    check_frame_layout(torch, m, frame, rows, split, mode, ref, keys, what, in_turn=True)


# ---------------------------------------------------------------------------- 1. primary outputs
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows", sc.HEIGHTS)
@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
def test_primary_outputs(torch, oracle_mod, contexts, frame, rows, mode):
    """All eight svo_frame outputs of every rank of every deal, twice in a row (the second launch is
    cost-ordered and, on a held view, re-splatted), band layout; then frame layout, every rank in turn into one
    frame.  A rank without rows returns SVO_OK and writes nothing."""
    m = contexts()
    ref = sc.oracle_frame(oracle_mod, frame, mode)
    set_view(m, frame)
    for split in sc.SPLITS:
        check_deal(torch, m, frame, rows, split, mode, ref, sc.FRAME_KEYS, f"{frame} {rows} {split} mode {mode}")


# ---------------------------------------------------------------------------- 2. policies
POLICIES = [({"loop_form": 0}, "AB"), ({"loop_form": 1}, "AB"), ({"beam": 0}, "AB"), ({"fetch_all": 0}, "AB"),
            ({"tile_order": 0}, "AB"), ({"xcd_strips": 0}, "AB"), ({"seg_all": 4}, "B"), ({"seg_all": 8}, "B"),
            ({"seg_all": 8, "seg_scramble": 1}, "B")]


@pytest.mark.parametrize("config,frames", POLICIES, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else v)
def test_policies_do_not_matter(torch, oracle_mod, contexts, config, frames):
    """svo_config moves time, never bytes: the weighted three-rank deals at heights 3, 5 and 12 under each
    policy, the same comparison as test_primary_outputs."""
    m = contexts(**config)
    for frame in frames:
        set_view(m, frame)
        for mode in (0, 1):
            ref = sc.oracle_frame(oracle_mod, frame, mode)
            for rows in WEIGHTED_DEALS:
                check_deal(torch, m, frame, rows, "w3", mode, ref, sc.FRAME_KEYS, f"{config} {frame} {rows} w3 mode {mode}")


# ---------------------------------------------------------------------------- 3. shadow rays
SHADOW_CONFIGS = [{"shadow_form": 0}, {"shadow_form": 1, "shadow_order": 0}, {"shadow_form": 1, "shadow_order": 1},
                  {"shadow_form": 2}]
# with hit records; with compact records only; the display words alone; hit records beside the caller's masks
SHADOW_SETS = (("hits", "rgba", "rgba8", "compact", "rgb8"), ("compact", "rgb8"), ("rgba8",), ("hits", "rgba", "hitmask"))
SHADOW_HEIGHTS = (1, 3, 5, 12, 50)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
@pytest.mark.parametrize("config", SHADOW_CONFIGS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_shadow_rays(torch, oracle_mod, contexts, config, frame, mode):
    """SVO_OPT_SHADOW_RAYS under the three shadow forms: the fused launch, the second pass over tiles (in
    raster and in its own cost order) and the pass over the compacted hit list, whose list is built by
    pack_hits_kernel<true> from band-local masks.  Whole frame first, then every rank of every deal in both
    layouts, for each set of outputs (the forms pick their scratch by what the caller asked for)."""
    m = contexts(**config)
    ref = sc.oracle_frame(oracle_mod, frame, mode, shadows=True)
    set_view(m, frame)
    m.SetShadowRays(True)
    try:
        for keys in SHADOW_SETS:
            check_band_layout(torch, m, frame, None, mode, ref, keys, f"{config} {frame} whole mode {mode} {keys}", launches=2)
        for rows in SHADOW_HEIGHTS:
            for split in sc.SPLITS:
                for keys in SHADOW_SETS:
                    what = f"{config} {frame} {rows} {split} mode {mode} {keys}"
                    for r in sc.ranks(split):
                        check_band_layout(torch, m, frame, sc.band_of(rows, r, split), mode, ref, keys, f"{what} rank {r}")
                    check_frame_layout(torch, m, frame, rows, split, mode, ref, keys, what)
    finally:
        m.SetShadowRays(False)


# ---------------------------------------------------------------------------- 4. the passes behind the primary launch
def check_pass(torch, m, frame, mode, want, keys, what):
    """Whole frame first (the partial edge tiles of the pass), then the weighted three-rank deals at heights
    3 and 12, in both layouts."""
    check_band_layout(torch, m, frame, None, mode, want, keys, f"{what} whole", launches=2)
    for rows in (3, 12):
        for r in sc.ranks("w3"):
            check_band_layout(torch, m, frame, sc.band_of(rows, r, "w3"), mode, want, keys, f"{what} {rows} w3 rank {r}")
        check_frame_layout(torch, m, frame, rows, "w3", mode, want, keys, f"{what} {rows} w3")


def model_args(frame):
    w, h = sc.FRAMES[frame]
    return sc.POOL_NAME, sc.pool(), "edge", w, h


@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
def test_reflection(torch, oracle_mod, contexts, frame):
    """reflect_list_kernel: the colour outputs are reflect_util.expected_frame's rows; hits, compact, position,
    voxel and hitmask stay those of the render with the pass off (the oracle's primary frame)."""
    from tests import reflect_util as ru
    m = contexts()
    off = sc.oracle_frame(oracle_mod, frame, 0)
    want = sc.with_colours(oracle_mod, off, ru.expected_frame(oracle_mod, *model_args(frame)))
    assert want["rgba"].tobytes() != off["rgba"].tobytes()
    set_view(m, frame)
    m.SetReflection(*ru.DEFAULT)
    try:
        check_pass(torch, m, frame, 0, want, sc.FRAME_KEYS, f"reflection {frame}")
    finally:
        m.SetReflection(None)


# (n_rays, radius, variant, shadow rays)
AMBIENT_CASES = [(4, float("inf"), 3, False), (8, 16.0, 5, False), (4, float("inf"), 3, True)]


@pytest.mark.parametrize("n_rays,radius,variant,shadows", AMBIENT_CASES)
@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
def test_ambient(torch, oracle_mod, contexts, frame, n_rays, radius, variant, shadows):
    """ambient_list_kernel, also behind the shadow pass over the hit list (shadow_form 2)."""
    from tests import ambient_util as au
    m = contexts(shadow_form=2) if shadows else contexts()
    off = sc.oracle_frame(oracle_mod, frame, 0, shadows=shadows)
    rgba = au.expected_frame(oracle_mod, *model_args(frame), n_rays=n_rays, radius=radius, variant=variant, shadows=shadows)
    want = sc.with_colours(oracle_mod, off, rgba)
    assert want["rgba"].tobytes() != off["rgba"].tobytes()
    set_view(m, frame)
    m.SetShadowRays(shadows)
    m.SetAmbient(au.AMBIENT, n_rays, radius, variant)
    try:
        check_pass(torch, m, frame, 0, want, sc.FRAME_KEYS, f"ambient {n_rays} {radius} {variant} shadows {shadows} {frame}")
    finally:
        m.SetAmbient(None)
        m.SetShadowRays(False)


@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
def test_skybox(torch, oracle_mod, contexts, frame, reflect):
    """A caller's panorama over the misses (the sky fill reads band-local masks), alone and with reflection,
    whose bounce rays that miss take the same rule."""
    from tests import ambient_util as au
    from tests import reflect_util as ru
    from tests import sky_util as su
    m = contexts()
    tex = su.texture(37, 19)
    off = sc.oracle_frame(oracle_mod, frame, 0)
    if reflect:
        rgba, on_sky = su.expected_reflection_frame(oracle_mod, *model_args(frame), 0, *ru.DEFAULT, tex, True, False)
        assert on_sky >= 100
    else:
        rgba = au.expected_frame(oracle_mod, *model_args(frame), n_rays=0, texture=(tex, True, False))
    want = sc.with_colours(oracle_mod, off, rgba)
    miss = ~off["hit"]
    assert np.all((want["rgba"][miss] != off["rgba"][miss]).any(axis=1)), "a miss pixel kept the gradient's colour"
    set_view(m, frame)
    m.SetSkybox(tex, bilinear=True, clamp_v=False)
    if reflect:
        m.SetReflection(*ru.DEFAULT)
    try:
        check_pass(torch, m, frame, 0, want, sc.FRAME_KEYS, f"skybox reflect {reflect} {frame}")
    finally:
        m.SetReflection(None)
        m.SetSkybox(None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
def test_lod_depth_clamp(torch, oracle_mod, contexts, frame, mode):
    """SetLod(0, 2^-5) through the LOD kernels: every output equals the oracle's on the pool pruned at level 5."""
    from tests.lod_util import pruned
    m = contexts()
    cut = pruned(sc.pool(), 5)
    want = sc.oracle_frame(oracle_mod, frame, mode, svo=cut, name="menger7 pruned at 5")
    assert want["hits"].tobytes() != sc.oracle_frame(oracle_mod, frame, mode)["hits"].tobytes()
    set_view(m, frame)
    m.SetLod(0.0, 2.0 ** -5)
    try:
        check_pass(torch, m, frame, mode, want, sc.FRAME_KEYS, f"lod clamp {frame} mode {mode}")
    finally:
        m.SetLod(0.0, 0.0)


def test_lod_pixel_footprint(torch, oracle_mod, contexts):
    """coef = pixel_footprint(pixels = 8) on frame A: compact records, voxel keys and band-local hit masks are
    tests/lod_tracer.py's on the oracle's camera rays."""
    from raytracingtest_amd.lod import pixel_footprint
    from tests import lod_tracer
    frame, mode = "A", 0
    w, h = sc.FRAMES[frame]
    c2w, inv_proj = sc.edge_camera().uniforms(w, h)
    pair = (np.float32(pixel_footprint(inv_proj, h, 8)), np.float32(0.0))
    ocam = oracle_mod.make_camera(c2w, inv_proj, (0.5, 0.5), main_light())
    o, d = np.zeros((h * w, 3), np.float32), np.zeros((h * w, 3), np.float32)
    fn, po, pd, cp = oracle_mod.lib().orc_camera_ray, o.ctypes.data, d.ctypes.data, ctypes.byref(ocam)
    for i in range(h * w):
        fn(cp, i % w, i // w, w, h, po + 12 * i, pd + 12 * i)
    res = lod_tracer.trace(sc.pool(), o, d, mode, pair[0], pair[1])
    want = {"compact": np.ascontiguousarray(lod_tracer.compact_bytes(res)).view(np.uint8).reshape(h, w, 12),
            "voxel": np.ascontiguousarray(res["key"], np.uint64).reshape(h, w), "hit": np.asarray(res["hit"], bool).reshape(h, w)}
    plain = sc.oracle_frame(oracle_mod, frame, mode)
    assert want["hit"].sum() >= 400 and want["compact"].tobytes() != plain["compact"].tobytes()
    m = contexts()
    set_view(m, frame)
    m.SetLod(*pair)
    try:
        check_pass(torch, m, frame, mode, want, ("compact", "voxel", "hitmask"), "lod footprint A")
    finally:
        m.SetLod(0.0, 0.0)


# ---------------------------------------------------------------------------- 5. samples in flight
_samples = {}


def oracle_samples(oracle_mod, frame, S, seed):
    """(offsets [2 S, 2], the oracle's accumulation after S samples, after 2 S), once per case."""
    from tests.test_gpu_frame import _oracle_accumulated
    key = (frame, S, seed)
    if key not in _samples:
        w, h = sc.FRAMES[frame]
        offs = jitter_offsets(2 * S, seed=seed)
        first = _oracle_accumulated(oracle_mod, sc.pool(), sc.edge_camera(), w, h, offs[:S])
        second = _oracle_accumulated(oracle_mod, sc.pool(), sc.edge_camera(), w, h, offs[S:], acc=first.copy(), first=S)
        _samples[key] = (offs, first.reshape(h, w, 4), second.reshape(h, w, 4))
    return _samples[key]


@pytest.mark.parametrize("split", ["rr2", "w3"])
@pytest.mark.parametrize("rows", [3, 12])
def test_samples_in_flight(torch, oracle_mod, contexts, rows, split):
    """svo_render_samples, S = 3, frame A: the display rank blends its rows into a frame-layout accumulation,
    the others into band accumulations and send 3-byte RGB; the PART_RGB8 assemble equals the oracle's
    accumulation, packed -- and again after the accumulations are continued once."""
    frame, S = "A", 3
    w, h = sc.FRAMES[frame]
    offs, first, second = oracle_samples(oracle_mod, frame, S, 5)
    m = contexts()
    set_view(m, frame)
    count, owner = sc.SPLITS[split]
    ys = [sc.rows_of(h, sc.band_of(rows, r, split)) for r in range(count)]
    sizes = {"acc0": w * h * 16, "frame8": w * h * 4}
    for r in range(1, count):
        sizes[f"acc{r}"] = len(ys[r]) * w * 16
        sizes[f"part{r}"] = len(ys[r]) * w * 3
    arena = sc.Arena(torch, sizes)
    for k in sizes:
        if k.startswith("acc"):
            arena.zero(k)   # a fresh render target
    for step, want in enumerate((first, second)):
        o = offs[step * S:(step + 1) * S]
        m.render_samples(w, h, o, step * S, arena.ptr("acc0"), rgba8=arena.ptr("frame8"), layout=LAYOUT_FRAME,
                         band=sc.band_of(rows, 0, split))
        for r in range(1, count):
            m.render_samples(w, h, o, step * S, arena.ptr(f"acc{r}"), rgb8=arena.ptr(f"part{r}"), band=sc.band_of(rows, r, split))
        m.assemble_frame(w, h, [None] + [arena.ptr(f"part{r}") for r in range(1, count)], _lib.PART_RGB8, band_rows=rows,
                         rgba8=arena.ptr("frame8"), skip_part=0, owner=owner)
        m.synchronize()
        arena.fetch()
        what = f"samples {rows} {split} step {step}"
        words = oracle_mod.pack_rgba8(want).reshape(h, w)
        same(arena.get("frame8"), words, 4, f"{what}: assembled display words")
        acc0 = arena.get("acc0").view(np.float32).reshape(h, w, 4)
        same(acc0[ys[0]], want[ys[0]], 16, f"{what}: display rank's accumulation")
        other = np.setdiff1d(np.arange(h), ys[0])
        assert not acc0[other].any(), f"{what}: the display rank blended into other ranks' rows"
        for r in range(1, count):
            same(arena.get(f"acc{r}"), want[ys[r]], 16, f"{what}: rank {r}'s band accumulation")
            same(arena.get(f"part{r}"), words.view(np.uint8).reshape(h, w, 4)[ys[r]][:, :, :3], 3, f"{what}: rank {r}'s RGB part")
        arena.check_guards(what)


def test_samples_rank_without_rows_is_a_no_op(torch, contexts):
    frame = "B"
    w, h = sc.FRAMES[frame]
    m = contexts()
    set_view(m, frame)
    band = sc.band_of(50, 1, "rr2")
    assert len(sc.rows_of(h, band)) == 0
    arena = sc.Arena(torch, {"acc": 0, "rgba8": 0, "rgb8": 0})
    offs = jitter_offsets(3, seed=5)
    m.render_samples(w, h, offs, 0, arena.ptr("acc"), rgba8=arena.ptr("rgba8"), rgb8=arena.ptr("rgb8"), band=band)
    m.render_samples(w, h, offs, 3, arena.ptr("acc"), band=band)
    m.synchronize()
    arena.fetch().check_guards("samples of a rank without rows")


# ---------------------------------------------------------------------------- 6. parts and assembly
PART_KEYS = ("compact", "rgba8", "rgb8")
ASSEMBLED = {_lib.PART_COMPACT: ("hits", "rgba", "rgba8", "compact"), _lib.PART_RGBA8: ("rgba8",), _lib.PART_RGB8: ("rgba8",),
             _lib.PART_SPARSE_RGB8: ("rgba8",)}
PART_OF_FORMAT = {_lib.PART_COMPACT: "compact", _lib.PART_RGBA8: "rgba8", _lib.PART_RGB8: "rgb8", _lib.PART_SPARSE_RGB8: "sparse"}


@pytest.mark.parametrize("rows", sc.HEIGHTS)
@pytest.mark.parametrize("frame", sorted(sc.FRAMES))
def test_parts_and_assembly(torch, oracle_mod, contexts, frame, rows):
    """The one-process-per-GPU split: every rank renders compact, RGBA8 and RGB8 parts and a sparse part
    (masks at its head, then svo_pack_hits); svo_assemble_frame rebuilds the frame from each format, from all
    parts and with skip_part 0 around rank 0's rows rendered in place.  A rank without rows sends an empty
    part: a valid pointer to a guard-only buffer (the sparse one: its 4-byte count, 0)."""
    w, h = sc.FRAMES[frame]
    m = contexts()
    ref = sc.oracle_frame(oracle_mod, frame, 0)
    set_view(m, frame)
    for split, (count, owner) in sc.SPLITS.items():
        what = f"{frame} {rows} {split}"
        ys = [sc.rows_of(h, sc.band_of(rows, r, split)) for r in range(count)]
        sizes = {}
        for r in range(count):
            n = len(ys[r]) * w
            sizes.update({f"compact{r}": n * 12, f"rgba8{r}": n * 4, f"rgb8{r}": n * 3, f"dense{r}": n * 3,
                          f"sparse{r}": _lib.sparse_part_bytes(sc.n_tiles(w, len(ys[r])), n)})
        parts = sc.Arena(torch, sizes)
        for r in range(count):
            band = sc.band_of(rows, r, split)
            m.render_frame(w, h, band=band, **{k: parts.ptr(f"{k}{r}") for k in PART_KEYS})
            m.render_frame(w, h, band=band, rgb8=parts.ptr(f"dense{r}"), hitmask=parts.ptr(f"sparse{r}"))
            m.pack_hits(w, h, band, parts.ptr(f"dense{r}"), parts.ptr(f"sparse{r}"))
        frames = sc.Arena(torch, {f"{tag}{fmt}{k}": w * h * sc.ITEM[k] for tag in ("all", "skip") for fmt, keys in ASSEMBLED.items()
                                  for k in keys})
        for fmt, keys in ASSEMBLED.items():
            ptrs = [parts.ptr(f"{PART_OF_FORMAT[fmt]}{r}") for r in range(count)]
            m.assemble_frame(w, h, ptrs, fmt, band_rows=rows, owner=owner, **{k: frames.ptr(f"all{fmt}{k}") for k in keys})
            m.render_frame(w, h, band=sc.band_of(rows, 0, split), layout=LAYOUT_FRAME, **{k: frames.ptr(f"skip{fmt}{k}") for k in keys})
            m.assemble_frame(w, h, [None] + ptrs[1:], fmt, band_rows=rows, owner=owner, skip_part=0,
                             **{k: frames.ptr(f"skip{fmt}{k}") for k in keys})
        m.synchronize()
        parts.fetch()
        frames.fetch()
        for r in range(count):
            for k in PART_KEYS:
                same(parts.get(f"{k}{r}"), sc.expected_rows(ref, ys[r], k), sc.ITEM[k], f"{what} rank {r}: {k} part")
            want = sc.expected_sparse_part(ref["hit"][ys[r]], ref["rgb8"][ys[r]], w)
            got = parts.get(f"sparse{r}")
            nt = sc.n_tiles(w, len(ys[r]))
            assert int(got[12 * nt:12 * nt + 4].view(np.uint32)[0]) == want["count"], f"{what} rank {r}: sparse count"
            same(got[:8 * nt], want["masks"], 8, f"{what} rank {r}: sparse masks")
            same(got[8 * nt:12 * nt + 4], want["offsets"], 4, f"{what} rank {r}: sparse offsets")
            same(got[12 * nt + 4:12 * nt + 4 + 3 * want["count"]], want["rgb"], 3, f"{what} rank {r}: sparse RGB")
        parts.check_guards(f"{what}: parts")
        for tag in ("all", "skip"):
            for fmt, keys in ASSEMBLED.items():
                for k in keys:
                    same(frames.get(f"{tag}{fmt}{k}"), ref[k], sc.ITEM[k], f"{what}: {k} assembled from {PART_OF_FORMAT[fmt]} parts ({tag})")
        frames.check_guards(f"{what}: assembled frames")


# ---------------------------------------------------------------------------- 7. multi-device contexts
def check_multi_frame(torch, m, oracle_mod, frame, what):
    """Render (the host path), a display-only frame and one with hit records, all against the oracle."""
    w, h = set_view(m, frame)
    ref = sc.oracle_frame(oracle_mod, frame, 0)
    rgba, hits = m.Render(w, h)
    same(hits, ref["hits"], 24, f"{what}: svo_render hit records")
    same(rgba, ref["rgba"], 16, f"{what}: svo_render Result")
    arena = sc.Arena(torch, {"only8": w * h * 4, "hits": w * h * 24, "rgba": w * h * 16, "rgba8": w * h * 4, "compact": w * h * 12})
    m.render_frame(w, h, rgba8=arena.ptr("only8"), layout=LAYOUT_FRAME)
    m.render_frame(w, h, layout=LAYOUT_FRAME, **arena.ptrs(("hits", "rgba", "rgba8", "compact")))
    m.synchronize()
    arena.fetch()
    same(arena.get("only8"), ref["rgba8"], 4, f"{what}: display-only frame")
    for k in ("hits", "rgba", "rgba8", "compact"):
        same(arena.get(k), ref[k], sc.ITEM[k], f"{what}: {k} beside hit records")
    arena.check_guards(what)


@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("rows", [1, 3, 5, 12, 50])
def test_multi_device_context(torch, oracle_mod, rows, sparse):
    """svo_create_multi with band_rows off the tile height, three members on one device: round-robin, then
    svo_set_band_deal (0, 1, 1, 2, 1); frames A and B alternate, so the members' payloads regrow and shrink.
    At 50 rows members own nothing (frame B: all but the display member) and must not disturb the frame."""
    m = RaytracingMaster(devices=[0, 0, 0], band_rows=rows, capacity_nodes=len(sc.pool()), config={"sparse_payload": sparse})
    try:
        m.SetSVOBuffer(sc.pool())
        for owner in (None, sc.WEIGHTED):
            m.set_band_deal(owner)
            for frame in ("A", "B", "A", "B"):
                check_multi_frame(torch, m, oracle_mod, frame, f"multi {rows} sparse {sparse} owner {owner} {frame}")
    finally:
        m.close()


def test_multi_device_samples(torch, oracle_mod):
    """svo_render_samples on a three-member context with 3-row bands, S = 2, continued once."""
    frame, S = "A", 2
    w, h = sc.FRAMES[frame]
    offs, first, second = oracle_samples(oracle_mod, frame, S, 9)
    m = RaytracingMaster(devices=[0, 0, 0], band_rows=3, capacity_nodes=len(sc.pool()))
    try:
        m.SetSVOBuffer(sc.pool())
        for owner in (None, sc.WEIGHTED):
            m.set_band_deal(owner)
            set_view(m, frame)
            arena = sc.Arena(torch, {"acc": w * h * 16, "frame8": w * h * 4})
            arena.zero("acc")
            for step, want in enumerate((first, second)):
                m.render_samples(w, h, offs[step * S:(step + 1) * S], step * S, arena.ptr("acc"), rgba8=arena.ptr("frame8"),
                                 layout=LAYOUT_FRAME)
                m.synchronize()
                arena.fetch()
                same(arena.get("frame8"), oracle_mod.pack_rgba8(want), 4, f"multi samples owner {owner} step {step}")
                arena.check_guards(f"multi samples owner {owner} step {step}")
    finally:
        m.close()


# ---------------------------------------------------------------------------- 8. a guarded pool
@pytest.mark.parametrize("mode", [0, 1])
def test_guarded_pool(torch, oracle_mod, mode):
    """The cyclic pool of tests/guard_pools.py (the guarded loop) from its own pose at frame A, in 5-row bands
    over three ranks: the shadow pass over the hit list and the reflection pass, compared as
    tests/test_gpu_guard.py and tests/test_gpu_reflection.py compare whole frames."""
    from tests import guard_pools as gp
    from tests import reflect_util as ru
    frame = "A"
    w, h = sc.FRAMES[frame]
    nodes, att = gp.cyclic7()
    svo = SVOData(nodes=nodes, attachments=att)
    cam = gp.diagonal_camera()
    lit = sc.oracle_frame(oracle_mod, frame, mode, svo=svo, camera=cam, name="cyclic7")
    dark = sc.oracle_frame(oracle_mod, frame, mode, shadows=True, svo=svo, camera=cam, name="cyclic7")
    for ref in (lit, dark):
        gp.assert_case_inputs("cyclic7", ref["hits"].reshape(-1))
    assert np.count_nonzero(dark["hits"]["flags"] & gp.FLAG_SHADOW) >= 100
    m = RaytracingMaster(device=0, capacity_nodes=1 << 10, config={"shadow_form": 2})
    try:
        m.SetSVOBuffer(svo)
        set_view(m, frame, cam)
        m.SetShadowRays(True)
        seen = []
        for r in range(3):
            a = check_band_layout(torch, m, frame, (5, r, 3), mode, dark, ("hits", "rgba", "rgba8", "compact"), f"cyclic7 shadows rank {r}")
            seen.append(a.get("hits").view(HIT_DTYPE))
        gp.assert_case_inputs("cyclic7", np.concatenate(seen))   # bit 2 in the GPU's own records: the guarded kernel ran
        check_frame_layout(torch, m, frame, 5, "rr3", mode, dark, ("hits", "rgba", "rgba8", "compact"), "cyclic7 shadows")
        m.SetShadowRays(False)
        want = sc.with_colours(oracle_mod, lit, ru.expected_frame(oracle_mod, "cyclic7", svo, "diagonal", w, h, mode))
        assert want["rgba"].tobytes() != lit["rgba"].tobytes()
        m.SetReflection(*ru.DEFAULT)
        for r in range(3):
            check_band_layout(torch, m, frame, (5, r, 3), mode, want, sc.FRAME_KEYS, f"cyclic7 reflection rank {r}")
        check_frame_layout(torch, m, frame, 5, "rr3", mode, want, sc.FRAME_KEYS, "cyclic7 reflection")
    finally:
        m.close()
