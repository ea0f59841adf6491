"""Placed objects, scene shadows and scene lights on the GPU against float64 world geometry
(tests/scene_geometry_model.py), directly and not through the oracle-based scene model: svo_trace_scene in both
stack modes, with and without the terrain, raw and clamped; svo_render_frame with svo_set_objects on and off the
tile grid, beam starts on and off; the shadow bit of SVO_OPT_SCENE_SHADOWS against the float64 shadow ray;
svo_scene_light_rays -> svo_trace_scene against the float64 segments; and a point light's shadowed render
against its unshadowed and unlit renders.

The ico2 pool is built on the GPU (native_builder.build_mesh_svo) and must equal the CPU's, whose leaves the
model reads.  `python -m tests.test_gpu_scene_geometry` adds the GPU's figures to
profiles/scene_geometry_truth.json."""
import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, RaytracingMaster
from raytracingtest_amd import _lib
from tests import scene_geometry_model as sg
from tests.geometry_model import EXACT, HLSL
from tests.scene_geometry_util import (MODE_NAME, QUERY_CASES, QUERY_FAMILIES, SEGMENT_FAMILY, check_shadow_classes,
                                       light_render_case, light_segments_check, oracle_normals, update_record)

pytestmark = pytest.mark.gpu

RENDER_SIZES = ("camera", "camera_small")


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def make_master():
    """The module's one context: the four pools behind one another, the mesh pool built on the GPU."""
    from raytracingtest_amd import native_builder as nb
    from tests import voxelize_util as vu
    pools = sg.pools()
    pos, tri, depth = vu.mesh("ico2")
    mesh = nb.build_mesh_svo(pos, tri, depth + 1, colors=vu.vertex_colors(pos))
    cpu = pools["ico2"][0]
    assert mesh.format == cpu.format == 1 and mesh.childDescriptors.tobytes() == cpu.childDescriptors.tobytes() \
        and mesh.attachments.tobytes() == cpu.attachments.tobytes(), "the GPU's mesh pool is not the CPU's"
    m = RaytracingMaster(device=0, capacity_nodes=sg.n_nodes())
    for name in sg.POOL_NAMES:
        m.SetSVOBuffer(mesh if name == "ico2" else pools[name][0], pools[name][3])
    return m


@pytest.fixture(scope="module")
def master(torch):
    m = make_master()
    yield m
    m.close()


# ------------------------------------------------------------------------------- svo_trace_scene
def query_case(m, set_name, family, terrain):
    """Both stack modes, raw on and off: {mode name: figures}."""
    traced, model = sg.case(set_name, family, terrain)
    objs = sg.placements(set_name)
    out = {}
    for mode in (EXACT, HLSL):
        first = None
        for raw in (False, True):
            what = f"{set_name} {family} {MODE_NAME[mode]} terrain {terrain} raw {raw}"
            hits, ids, pos, vox = m.TraceScene(traced, objs, stack_mode=mode, raw=raw, terrain=terrain, want_position=True,
                                               want_voxel=True)
            fig = sg.scene_check(set_name, traced, mode, model, hits, ids, vox, pos, oracle_normals(), terrain=terrain, what=what)
            got = (hits.tobytes(), ids.tobytes(), pos.tobytes(), vox.tobytes())
            if first is None:
                first = got
            assert got == first, f"{what}: differs from the clamped query (no component is small enough to clamp)"
        assert fig["hits"] >= 200 and fig["self_hits"] == 0
        out[MODE_NAME[mode]] = fig
    return out


@pytest.mark.parametrize("set_name,family,terrain", QUERY_CASES)
def test_trace_scene_against_geometry(torch, oracle_mod, master, set_name, family, terrain):
    print(set_name, family, terrain, query_case(master, set_name, family, terrain))


# ---------------------------------------------------------------------------------------- renders
ITEM = {"hits": 24, "position": 16, "voxel": 8, "rgba": 16}


def render(torch, m, w, h, mode, keys=("hits", "position", "voxel")):
    """One svo_render_frame into 0xEE-filled device buffers: hits as records, position [n, 4] f32, voxel keys,
    rgba as 16 bytes per pixel."""
    b = {k: torch.full((w * h * ITEM[k],), 0xEE, dtype=torch.uint8, device="cuda") for k in keys}
    torch.cuda.synchronize()
    m.render_frame(w, h, stack_mode=mode, **{k: v.data_ptr() for k, v in b.items()})
    m.synchronize()
    got = {k: v.cpu().numpy() for k, v in b.items()}
    view = {"hits": lambda a: a.view(HIT_DTYPE), "position": lambda a: a.view(np.float32).reshape(-1, 4),
            "voxel": lambda a: a.view(np.uint64), "rgba": lambda a: a.reshape(-1, 16)}
    return {k: view[k](a) for k, a in got.items()}


def setup(m, family, shadows=False, lights=None):
    w, h = sg.CAM_SIZES[family]
    m.UpdateShaderParameters(sg.camera(), w, h, light=np.asarray(sg.LIGHT, np.float32))
    m.SetSceneShadows(True)
    m.SetShadowRays(shadows)
    m.SetLights(lights)
    m.SetObjects(sg.placements("scene"))
    return w, h


def reset(m):
    m.set_config(beam=1)
    m.SetShadowRays(False)
    m.SetLights(None)
    m.SetObjects(None)
    m.SetSceneShadows(False)


def render_case(torch, m, family):
    """A frame with svo_set_objects, beam starts on and off, both stack modes: the object pass against section 3."""
    traced, model = sg.case("scene", family)
    out = {}
    try:
        w, h = setup(m, family)
        for beam in (1, 0):
            m.set_config(beam=beam)
            for mode in (EXACT, HLSL):
                what = f"rendered {family} beam {beam} {MODE_NAME[mode]}"
                got = render(torch, m, w, h, mode)
                ids = sg.ids_of_records("scene", traced, got["hits"], model)
                fig = sg.scene_check("scene", traced, mode, model, got["hits"], ids, got["voxel"], got["position"],
                                     oracle_normals(), what=what)
                assert min(fig["hits_per_candidate"]) >= 20, f"{what}: hits per candidate {fig['hits_per_candidate']}"
                out[f"beam{beam}_{MODE_NAME[mode]}"] = fig
    finally:
        reset(m)
    return out


@pytest.mark.parametrize("family", RENDER_SIZES)
def test_rendered_objects_against_geometry(torch, oracle_mod, master, family):
    print(family, render_case(torch, master, family))


def shadow_case(torch, m, family):
    traced, model = sg.case("scene", family)
    out = {}
    try:
        w, h = setup(m, family, shadows=True)
        for mode in (EXACT, HLSL):
            what = f"scene shadow {family} {MODE_NAME[mode]}"
            got = render(torch, m, w, h, mode)
            ids = sg.ids_of_records("scene", traced, got["hits"], model)
            sg.scene_check("scene", traced, mode, model, got["hits"], ids, got["voxel"], got["position"], oracle_normals(),
                           extra_flags=8, what=what)
            fig = sg.shadow_check("scene", traced, got["hits"], ids, sg.LIGHT, mode, what=what)
            if family == "camera":
                check_shadow_classes(fig, what)
            out[MODE_NAME[mode]] = fig
    finally:
        reset(m)
    return out


@pytest.mark.parametrize("family", RENDER_SIZES)
def test_scene_shadow_bit_against_geometry(torch, oracle_mod, master, family):
    print(family, shadow_case(torch, master, family))


# ----------------------------------------------------------------------------------- point lights
def light_query_case(m, mode):
    traced, _ = sg.case("scene", SEGMENT_FAMILY)
    objs = sg.placements("scene")
    hits, ids, _, vox = m.TraceScene(traced, objs, stack_mode=mode, raw=True, want_voxel=True)
    segments = m.SceneLightRays(traced, hits, vox, ids, objs, list(sg.LIGHTS), raw=True)

    def trace(rays):
        return m.TraceScene(rays, objs, stack_mode=mode, want_position=True, want_voxel=True)

    def reorder(rays):
        h2, i2, p2, v2 = trace(rays)
        return h2, i2, v2, p2
    return light_segments_check(traced, hits, ids, segments, reorder, mode, f"light segments {MODE_NAME[mode]}")


def test_light_segments_against_geometry(torch, oracle_mod, master):
    for mode in (EXACT, HLSL):
        print(MODE_NAME[mode], light_query_case(master, mode))


def light_render_figures(torch, m, light, mode):
    """Three renders of the camera family for one light: none, unshadowed, shadowed."""
    traced, model = sg.case("scene", "camera")
    pos, rng, col = sg.LIGHTS[light]
    keys = ("hits", "voxel", "rgba")
    try:
        w, h = setup(m, "camera")
        base = render(torch, m, w, h, mode, keys)
        m.SetLights([(pos, rng, col, _lib.LIGHT_NO_SHADOW)])
        plain = render(torch, m, w, h, mode, keys)
        m.SetLights([(pos, rng, col)])
        shadowed = render(torch, m, w, h, mode, keys)
    finally:
        reset(m)
    for other in (plain, shadowed):
        assert other["hits"].tobytes() == base["hits"].tobytes() and other["voxel"].tobytes() == base["voxel"].tobytes()
    ids = sg.ids_of_records("scene", traced, base["hits"], model)
    contributes = (base["rgba"] != plain["rgba"]).any(axis=1)
    px, must, clear, on_o, fig = light_render_case(traced, base["hits"], ids, sg.LIGHTS[light], mode, contributes)
    what = f"light {light} {MODE_NAME[mode]}"
    dark = (shadowed["rgba"][px] == base["rgba"][px]).all(axis=1)
    lit = (shadowed["rgba"][px] == plain["rgba"][px]).all(axis=1)
    assert dark[must].all(), f"{what}: {np.count_nonzero(~dark[must])} pixels whose segment must be occluded are lit, first {px[must & ~dark][:5]}"
    assert lit[clear].all(), f"{what}: {np.count_nonzero(~lit[clear])} pixels whose segment meets nothing are dark, first {px[clear & ~lit][:5]}"
    assert (dark | lit).all(), f"{what}: a pixel that is neither the lit nor the unlit one"
    fig.update(undecided=int((~must & ~clear).sum()), undecided_dark=int(dark[~must & ~clear].sum()))
    return fig


@pytest.mark.parametrize("light", range(len(sg.LIGHTS)))
def test_light_renders_against_geometry(torch, oracle_mod, master, light):
    for mode in (EXACT, HLSL):
        print(light, MODE_NAME[mode], light_render_figures(torch, master, light, mode))


# ------------------------------------------------------------------------------------- the record
def gpu_record():
    import torch
    m = make_master()
    rec = {}
    try:
        for set_name in QUERY_FAMILIES:
            entry = {"trace_scene": {}}
            for s_, f, t in QUERY_CASES:
                if s_ == set_name:
                    entry["trace_scene"].setdefault(f, {})[f"terrain_{int(t)}"] = query_case(m, set_name, f, t)
            if set_name == "scene":
                entry["render_frame"] = {f: render_case(torch, m, f) for f in RENDER_SIZES}
                entry["shadow"] = {f: shadow_case(torch, m, f) for f in RENDER_SIZES}
                entry["light_segments"] = {MODE_NAME[mode]: light_query_case(m, mode) for mode in (EXACT, HLSL)}
                entry["light_renders"] = {str(j): {MODE_NAME[mode]: light_render_figures(torch, m, j, mode) for mode in (EXACT, HLSL)}
                                          for j in range(len(sg.LIGHTS))}
            rec[set_name] = entry
    finally:
        m.close()
    return rec


if __name__ == "__main__":
    import sys
    update_record("gpu", gpu_record(), *sys.argv[1:2])
