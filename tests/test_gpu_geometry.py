"""GPU traversal against float64 geometry (tests/geometry_model.py), directly and not through the oracle:
svo_trace_rays in both stack modes, unordered and ordered, on deep, sparse, mixed-depth and dense pools and
every ray family; the camera family rendered by svo_render_frame with beam starts on and off; and the shadow
bit of SVO_OPT_SHADOW_RAYS against the float64 shadow ray.

`python -m tests.test_gpu_geometry` adds the GPU's figures to profiles/geometry_truth.json."""
import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, RaytracingMaster
from raytracingtest_amd.camera import main_light
from tests import geometry_model as gm
from tests.geometry_model import EXACT, HLSL
from tests.query_util import pack_mask
from tests.test_geometry_model import MODE_NAME, MUST_POOLS, NO_MUST, update_record

pytestmark = pytest.mark.gpu

RENDER_POOLS = ("walk12", "walk16", "mixed")
SHADOW_POOLS = ("walk12", "menger7")


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


class Contexts:
    """One context per pool, made on first use and kept for the module."""

    def __init__(self):
        self.made = {}

    def __call__(self, name):
        if name not in self.made:
            svo = gm.pool(name)[0]
            m = RaytracingMaster(device=0, capacity_nodes=len(svo))
            m.SetSVOBuffer(svo)
            self.made[name] = m
        return self.made[name]

    def close(self):
        for m in self.made.values():
            m.close()
        self.made = {}


@pytest.fixture(scope="module")
def ctx(torch):
    c = Contexts()
    yield c
    c.close()


def query(torch, m, traced, mode, ordered):
    """svo_trace_rays of rays as traced: (hit records, voxel keys); the hit mask must equal the records' hit bits."""
    from tests.test_gpu_query import trace
    got = trace(torch, m, traced, mode=mode, ordered=ordered, outputs=("hits", "voxel", "hitmask"))
    hits = got["hits"].view(HIT_DTYPE)
    assert got["hitmask"].tobytes() == pack_mask((hits["flags"] & 1) != 0).tobytes(), "hit mask != the records' hit bits"
    return hits, got["voxel"].view("<u8")


def query_case(torch, m, name, family):
    """Every stack mode and order of one pool and family against section 2: {mode name: figures}."""
    traced, _, summary = gm.case(name, family)
    out = {}
    for mode in (EXACT, HLSL):
        first = None
        for ordered in (False, True):
            what = f"{name} {family} {MODE_NAME[mode]} ordered {ordered}"
            hits, vox = query(torch, m, traced, mode, ordered)
            fig = gm.check(name, traced, mode, summary[mode], hits, vox, what=what)
            if first is None:
                first = hits.tobytes(), vox.tobytes()
            assert (hits.tobytes(), vox.tobytes()) == first, f"{what}: differs from the unordered query"
        if name in MUST_POOLS and (name, family, mode) not in NO_MUST:
            assert fig["hits"] >= 200
        out[MODE_NAME[mode]] = fig
        out[MODE_NAME[mode] + "_records"] = hits
    lost = ((out["exact_records"]["flags"] & 1) != 0) & ((out["hlsl_records"]["flags"] & 1) == 0)
    for k in ("exact_records", "hlsl_records"):
        del out[k]
    out["exact_hit_hlsl_miss"] = int(lost.sum())
    return out


@pytest.mark.parametrize("family", gm.FAMILIES)
@pytest.mark.parametrize("name", gm.POOLS)
def test_trace_rays_against_geometry(torch, ctx, name, family):
    print(name, family, query_case(torch, ctx(name), name, family))


def render(torch, m, w, h, mode):
    hits = torch.full((w * h * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    vox = torch.full((w * h,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m.render_frame(w, h, hits=hits.data_ptr(), voxel=vox.data_ptr(), stack_mode=mode)
    m.synchronize()
    return hits.cpu().numpy().view(HIT_DTYPE), vox.cpu().numpy().view(np.uint64)


def render_case(torch, m, name):
    """The camera family as a rendered 128 x 96 frame, beam starts on and off, both stack modes."""
    rays, _ = gm.family_rays(name, "camera")
    traced, _, summary = gm.case(name, "camera")
    assert traced.tobytes() == rays.tobytes()        # no component below 2^-23: the frame traces these very rays
    w, h = gm.cam_size(name)
    out = {}
    try:
        for beam in (1, 0):
            m.set_config(beam=beam)
            m.UpdateShaderParameters(gm.camera(name), w, h)
            starts = torch.full((w * h,), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            m.beam_starts_device(w, h, starts.data_ptr())
            m.synchronize()
            st = starts.cpu().numpy()
            for mode in (EXACT, HLSL):
                what = f"{name} rendered beam {beam} {MODE_NAME[mode]}"
                hits, vox = render(torch, m, w, h, mode)
                fig = gm.check(name, traced, mode, summary[mode], hits, vox, what=what)
                hit = (hits["flags"] & 1) != 0
                fig["beam_started_hits"] = int((hit & np.isfinite(st)).sum())
                if beam:
                    assert fig["beam_started_hits"] > 0, f"{what}: no hit ray took a beam start"
                    assert not np.any(hit & np.isfinite(st) & (st > hits["t"].astype(np.float64) / 2048.0)), \
                        f"{what}: a start past its ray's hit"
                else:
                    assert fig["beam_started_hits"] == 0, f"{what}: beam starts with beam off"
                out[f"beam{beam}_{MODE_NAME[mode]}"] = fig
    finally:
        m.set_config(beam=1)
    return out


@pytest.mark.parametrize("name", RENDER_POOLS)
def test_rendered_camera_frame_against_geometry(torch, ctx, name):
    print(name, render_case(torch, ctx(name), name))


def shadow_case(torch, m, name):
    rays, _ = gm.family_rays(name, "camera")
    w, h = gm.cam_size(name)
    out = {}
    m.UpdateShaderParameters(gm.camera(name), w, h)
    m.SetShadowRays(True)
    try:
        for mode in (EXACT, HLSL):
            hits, _ = render(torch, m, w, h, mode)
            fig = gm.check_shadow(name, rays, hits, main_light(), mode, what=f"{name} shadow {MODE_NAME[mode]}")
            assert fig["must_shadowed"] >= 20 and fig["must_lit"] >= 20
            out[MODE_NAME[mode]] = fig
    finally:
        m.SetShadowRays(False)
    return out


@pytest.mark.parametrize("name", SHADOW_POOLS)
def test_shadow_bit_against_geometry(torch, ctx, name):
    print(name, shadow_case(torch, ctx(name), name))


def gpu_record():
    import torch
    c = Contexts()
    rec = {}
    try:
        for name in gm.POOLS:
            rec[name] = {"trace_rays": {f: query_case(torch, c(name), name, f) for f in gm.FAMILIES}}
            if name in RENDER_POOLS:
                rec[name]["render_frame"] = render_case(torch, c(name), name)
            if name in SHADOW_POOLS:
                rec[name]["shadow"] = shadow_case(torch, c(name), name)
    finally:
        c.close()
    return rec


if __name__ == "__main__":
    import sys
    update_record("gpu", gpu_record(), *sys.argv[1:2])
