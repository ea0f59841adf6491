"""The staging the _host ray-batch calls share (svo_rt.hip HostStage): one context, every family's host call in a
row at sizes that cross a 64-lane wave (63, 65, 129) and hit n = 1, so that the one staging buffer grows, grows
again for the largest stage (the 16-ray ambient fan-out) and is then used at every fraction of its size; one
ordered device query on another stream in between makes the next host call wait for that stream first.  Every result
equals, byte for byte, what the family's own GPU test compares with: numpy's statement of the rule, or for the
two traces the same call's device path on the same rays."""
import numpy as np
import pytest

from raytracingtest_amd import HIT_DTYPE, RaytracingMaster, sky
from raytracingtest_amd.ambient import ambient_rays
from raytracingtest_amd.lights import light_rays
from raytracingtest_amd.objects import object_rays
from raytracingtest_amd.reflection import bounce_rays
from tests import light_util as lu
from tests import object_util as ou
from tests import sky_util as su
from tests.lod_util import pools
from tests.query_util import random_batch
from tests.test_gpu_reflection import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def device_trace(torch, m, rays, stream=None, ordered=False):
    """svo_trace_rays on device buffers: (hits, position, voxel) as TraceRays returns them."""
    n = len(rays)
    d_rays = dev(torch, rays)
    bufs = [torch.zeros(n * item, dtype=torch.uint8, device="cuda") for item in (24, 16, 8)]
    torch.cuda.synchronize()
    m.trace_rays_device(d_rays.data_ptr(), n, hits=bufs[0].data_ptr(), position=bufs[1].data_ptr(),
                        voxel=bufs[2].data_ptr(), ordered=ordered, stream=None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()   # not svo_synchronize: the context must remember which stream used its scratch last
    h, p, v = (b.cpu().numpy() for b in bufs)
    return h.view(HIT_DTYPE), p.view(np.float32).reshape(n, 4), v.view(np.uint64)


def device_scene(torch, m, rays, objects):
    n = len(rays)
    d_rays = dev(torch, rays)
    bufs = [torch.zeros(n * item, dtype=torch.uint8, device="cuda") for item in (24, 16, 8, 4)]
    torch.cuda.synchronize()
    m.trace_scene_device(d_rays.data_ptr(), n, objects, hits=bufs[0].data_ptr(), position=bufs[1].data_ptr(),
                         voxel=bufs[2].data_ptr(), object_id=bufs[3].data_ptr())
    torch.cuda.synchronize()
    h, p, v, i = (b.cpu().numpy() for b in bufs)
    return h.view(HIT_DTYPE), i.view(np.int32), p.view(np.float32).reshape(n, 4), v.view(np.uint64)


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), f"{what}: output {k}"


def test_every_host_call_in_a_row_on_one_context(torch, text_svo):
    scene = ou.Scene(pools(text_svo))          # tree7 at root 0, the objects' trees behind it
    objects = ou.object_set(scene, "two")
    eight = lu.SETS["eight"]
    tex = su.texture(37, 19)
    rays = np.ascontiguousarray(random_batch()[:129])
    m = RaytracingMaster(device=0, capacity_nodes=1 << 16)
    side = torch.cuda.Stream()
    try:
        scene.upload(m)
        m.SetSkybox(tex)

        # 1. a trace with every output, n = 129
        traced = m.TraceRays(rays, want_position=True, want_voxel=True)
        same(traced, device_trace(torch, m, rays), "TraceRays, n = 129")
        hits, _, vox = traced
        hit = (hits["flags"] & 1) != 0
        # both kinds of record in every later step (the oracle counts 23 hits, 11 among the first 65)
        assert hit.sum() >= 10 and hit[:65].sum() >= 5 and (~hit[:65]).sum() >= 5, int(hit.sum())

        # 2. bounce rays in place in the stage, n = 129
        same([m.BounceRays(rays, hits, vox)], [bounce_rays(rays, hits, vox)], "BounceRays, n = 129")

        # 3. the largest stage: 65 entries with 16 ambient rays each
        same([m.AmbientRays(rays[:65], hits[:65], vox[:65], 16, 4.0, 5)],
             [ambient_rays(rays[:65], hits[:65], vox[:65], 16, 4.0, 5)], "AmbientRays, 16 x 65")

        # 4. eight lights, n = 65
        same([m.LightRays(rays[:65], hits[:65], vox[:65], eight)], [light_rays(rays[:65], hits[:65], vox[:65], eight)],
             "LightRays, 8 x 65")

        # an ordered device query on another stream takes the query scratch over: the next host call must wait for it
        same(device_trace(torch, m, rays, stream=side, ordered=True), traced, "ordered device query on a second stream")

        # 5. one ray in an object's frame
        same([m.ObjectRays(rays[:1], objects[0])], [object_rays(rays[:1], objects[0])], "ObjectRays, n = 1")

        # 6. a scene query with two objects and every output, n = 63
        same(m.TraceScene(rays[:63], objects, want_position=True, want_voxel=True), device_scene(torch, m, rays[:63], objects),
             "TraceScene, n = 63")

        # 7. the sky sampler, n = 65
        d4 = np.zeros((65, 4), np.float32)
        d4[:, :3] = rays["dir"][:65]
        want = np.ones((65, 4), np.float32)
        want[:, :3] = sky.sample_sky(d4, tex, True, False)
        same([m.SampleSky(d4)], [want], "SampleSky, n = 65")

        # 8. a trace again, n = 1: the stage at a fraction of its size
        same(m.TraceRays(rays[:1], want_position=True, want_voxel=True), device_trace(torch, m, rays[:1]), "TraceRays, n = 1")

        # 9. ambient rays again, 4 x 129
        same([m.AmbientRays(rays, hits, vox, 4, float("inf"), 0)], [ambient_rays(rays, hits, vox, 4, float("inf"), 0)],
             "AmbientRays, 4 x 129")
    finally:
        m.forget_stream(side.cuda_stream)
        m.close()
