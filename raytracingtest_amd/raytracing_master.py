"""Host-side mirror of the reference's `RaytracingMaster` MonoBehaviour
(Assets/Scripts/SVO/GPU/RaytracingMaster.cs) over the C-ABI of libsvo_rt.so.

Same names and argument meaning as the reference:
  InitializeSVOBuffer()          RaytracingMaster.cs:111-116
  SetSVOBuffer(data, offset=0)   RaytracingMaster.cs:118-135 (public overload)
  SetSVOBuffer()                 RaytracingMaster.cs:90-109  (rebuild from maxLevel / sampleType)
  UpdateShaderParameters(...)    RaytracingMaster.cs:32-41
  Render(width, height)          RaytracingMaster.cs:60-74   (Dispatch + result)
  accumulate_device(...)         RaytracingMaster.cs:70-73 + AddShader.shader (Blit with _Sample,
                                 then _currentSample++; reset to 0 when the camera moves, :44-47)
  RenderProgressive(width, height)  OnRenderImage end to end (:55-74): one sample rendered,
                                 accumulated on the device, display RGBA8 to the host
Beyond the reference (one GPU, one Dispatch):
  RaytracingMaster(devices=[0, 1, ...])  one context over several GPUs of the node
                                 (svo_create_multi): SVO replica per GPU, the frame
                                 rendered in row bands and gathered to devices[0]
  render_frame(...)              every per-pixel output (hits, Result, RGBA8,
                                 compact records, hit position, voxel key)
  assemble_frame(...)            rebuild a frame from band parts (the display side
                                 of the one-process-per-GPU split)
  TraceRays(origins, dirs)       caller-supplied ray batches (the reference's CPU-side
  trace_rays_device(...)         SVO.Trace(Ray), Interfaces.cs:6-15) on the GPU
  OverlapVolumes(shapes)         which voxels boxes and spheres touch (no reference counterpart)
  overlap_volumes_device(...)
  ClosestVoxels(queries)         the nearest voxel to a point, its squared distance and the closest point
  closest_voxels_device(...)     on it (no reference counterpart)
Errors surface as SvoError (the C-ABI status + svo_last_error text) instead of
Unity's silent shader failures.  There is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import HIT_DTYPE, LAYOUT_BAND, LAYOUT_FRAME, STACK_EXACT, STACK_HLSL, SvoError, SvoFrame, check, make_band
from .camera import column_major, main_camera, main_light
from .query import batch_arrays
from .svo_data import SVOData

# RaytracingMaster.cs:113-115: "one gibibyte of memory" / 8 elements of 4 bytes
REFERENCE_CAPACITY = 1073741824 // 8


def _frame(hits=None, rgba=None, rgba8=None, compact=None, position=None, voxel=None, layout=LAYOUT_BAND, rgb8=None,
           hitmask=None):
    return SvoFrame(hits, rgba, rgba8, compact, position, voxel, rgb8, hitmask, layout)


class RaytracingMaster:
    def __init__(self, device=0, capacity_nodes=REFERENCE_CAPACITY, maxLevel=5, sampleType=4, devices=None,
                 band_rows=8, config=None):
        """devices: list of HIP device indices for a multi-device context (devices[0]
        displays; an index may repeat); None = the single device `device`.
        config: svo_config fields to set on the new context (set_config)."""
        self.devices = None if devices is None else [int(d) for d in devices]
        self.device = device if devices is None else self.devices[0]
        self.band_rows = int(band_rows)
        self.capacity_nodes = int(capacity_nodes)
        self.maxLevel = maxLevel        # [Range(1, 8)] in the reference (:16-17)
        self.sampleType = sampleType    # SampleFunctions.Type.Custom1 = 4 (:18)
        self._ctx = ctypes.c_void_p()
        self._camera_set = False
        self._c2w = None
        self._options = 0               # svo_set_options bits
        self.currentSample = 0          # _currentSample (RaytracingMaster.cs:12)
        self._config = dict(config or {})
        self.InitializeSVOBuffer()

    # ------------------------------------------------------------------ setup
    def InitializeSVOBuffer(self):
        L = _lib.lib()
        if self._ctx:
            L.svo_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()
        if self.devices is None:
            check(L.svo_create(self.device, self.capacity_nodes, ctypes.byref(self._ctx)), "svo_create")
        else:
            arr = (ctypes.c_int * len(self.devices))(*self.devices)
            check(L.svo_create_multi(arr, len(self.devices), self.capacity_nodes, self.band_rows,
                                     ctypes.byref(self._ctx)), "svo_create_multi")
        self._options = 0
        if self._config:
            self.set_config(**self._config)

    def get_config(self):
        """The context's svo_config (render policy) as a dict."""
        c = _lib.SvoConfig()
        c.size = ctypes.sizeof(_lib.SvoConfig)
        check(_lib.lib().svo_get_config(self._ctx, ctypes.byref(c)), "svo_get_config")
        return c.to_dict()

    def set_config(self, **fields):
        """Change svo_config fields (include/svo_rt.h; the counterpart of RaytracingMaster's Inspector
        fields, RaytracingMaster.cs:16-18): the others keep their values.  Policy only -- every
        setting renders the same frames."""
        c = _lib.SvoConfig()
        c.size = ctypes.sizeof(_lib.SvoConfig)
        check(_lib.lib().svo_get_config(self._ctx, ctypes.byref(c)), "svo_get_config")
        names = {n for n, _ in _lib.CONFIG_FIELDS}
        for k, v in fields.items():
            if k not in names:
                raise SvoError(f"svo_config has no field {k!r}")
            setattr(c, k, v)
        check(_lib.lib().svo_set_config(self._ctx, ctypes.byref(c)), "svo_set_config")
        self._config.update(fields)

    def SetSVOBuffer(self, data=None, offset=0):
        """Upload an SVOData at descriptor `offset`; with no data, build one from
        (sampleType, maxLevel) like the private reference overload."""
        if data is None:
            from .builder import build_svo_for_sampler
            data = build_svo_for_sampler(self.sampleType, self.maxLevel)
        if not isinstance(data, SVOData):
            raise TypeError("SetSVOBuffer expects an SVOData")
        L = _lib.lib()
        att = np.ascontiguousarray(data.attachments, np.uint32)
        if data.format == 1:
            desc = np.ascontiguousarray(data.childDescriptors, np.int32)
            check(L.svo_set_buffer(self._ctx, desc.ctypes.data, len(desc), att.ctypes.data, len(att), int(offset)),
                  "svo_set_buffer")
        else:
            nodes = np.ascontiguousarray(data.nodes, np.uint64)
            check(L.svo_set_buffer_v2(self._ctx, nodes.ctypes.data, len(nodes), att.ctypes.data, len(att),
                                      int(offset)), "svo_set_buffer_v2")
        return data

    def UpdateShaderParameters(self, camera=None, width=1920, height=1080, pixel_offset=(0.5, 0.5), light=None):
        """camera: raytracingtest_amd.camera.Camera, or a (c2w, inv_proj) pair of 4x4 arrays."""
        camera = main_camera() if camera is None else camera
        if isinstance(camera, tuple):
            c2w, inv_proj = camera
        else:
            c2w, inv_proj = camera.uniforms(width, height)
        light = main_light() if light is None else np.asarray(light, np.float32)
        c2w = np.asarray(c2w, np.float32)
        if self._c2w is None or not np.array_equal(self._c2w, c2w):   # transform.hasChanged (:44-47)
            self.currentSample = 0
            self._c2w = c2w.copy()
        c = column_major(c2w)
        p = column_major(inv_proj)
        lt = np.ascontiguousarray(light, np.float32)
        check(_lib.lib().svo_set_camera(self._ctx, c.ctypes.data, p.ctypes.data, float(pixel_offset[0]),
                                        float(pixel_offset[1]), lt.ctypes.data), "svo_set_camera")
        self._camera_set = True

    def _set_option(self, bit, enable):
        self._options = (self._options | bit) if enable else (self._options & ~bit)
        check(_lib.lib().svo_set_options(self._ctx, self._options), "svo_set_options")

    def SetShadowRays(self, enable=True):
        """Trace one shadow ray per primary hit toward -_DirectionalLight (the
        reference's commented-out test, RaytraceCompute.compute:105-112)."""
        self._set_option(_lib.SVO_OPT_SHADOW_RAYS, enable)

    def SetSceneShadows(self, enable=True):
        """Let the shadow pass (SetShadowRays) and the light pass (SetLights) of a render know the placed
        objects (SetObjects): objects cast and receive shadows (SVO_OPT_SCENE_SHADOWS; scene_light.py is the
        rule).  Off by default: a render with objects then refuses shadow rays and lights.  Without objects
        the option changes nothing."""
        self._set_option(_lib.SVO_OPT_SCENE_SHADOWS, enable)

    def SetLod(self, ray_size_coef, ray_size_bias=0.0):
        """Level-of-detail termination of the primary rays (svo_set_lod; Laine-Karras's test, commented
        out at NVIDIASVO.compute:77-79): a voxel whose side is at most tc_max * ray_size_coef +
        ray_size_bias ends the walk like a leaf.  ray_size_coef: lod.pixel_footprint(inv_proj, height,
        pixels); ray_size_bias in SVO units (a world length / 32).  (0, 0): off, the default."""
        before = self.GetLod()
        check(_lib.lib().svo_set_lod(self._ctx, float(ray_size_coef), float(ray_size_bias)), "svo_set_lod")
        if self.GetLod() != before:   # another image: the accumulation restarts, as after a camera move
            self.currentSample = 0

    def GetLod(self):
        """(ray_size_coef, ray_size_bias) of the context (svo_get_lod)."""
        c, b = ctypes.c_float(), ctypes.c_float()
        check(_lib.lib().svo_get_lod(self._ctx, ctypes.byref(c), ctypes.byref(b)), "svo_get_lod")
        return c.value, b.value

    def SetReflection(self, specular, max_bounces=7):
        """Specular reflection bounces of the renders (svo_set_reflection; the reference's Trace /
        Shade loop, RaytraceCompute.compute:159-166, with a non-zero `specular`): each hit pixel's
        colour becomes the primary colour plus, per bounce b <= max_bounces (0..7), specular^b times
        the colour the bounce ray finds (reflection.bounce_rays is the rule).  specular: three
        numbers in [0, 1], or None for off (the default).  Only the colour outputs change."""
        before = self.GetReflection()
        if specular is None:
            check(_lib.lib().svo_set_reflection(self._ctx, None, 0), "svo_set_reflection")
        else:
            s = (ctypes.c_float * 3)(*[float(v) for v in specular])
            check(_lib.lib().svo_set_reflection(self._ctx, s, int(max_bounces)), "svo_set_reflection")
        if self.GetReflection() != before:   # another image: the accumulation restarts
            self.currentSample = 0

    def GetReflection(self):
        """((r, g, b) specular, max_bounces) of the context (svo_get_reflection)."""
        s, n = (ctypes.c_float * 3)(), ctypes.c_int()
        check(_lib.lib().svo_get_reflection(self._ctx, s, ctypes.byref(n)), "svo_get_reflection")
        return (s[0], s[1], s[2]), n.value

    def SetAmbient(self, ambient, n_rays=4, radius=float("inf"), variant=0):
        """Sky light with ambient occlusion (svo_set_ambient; ambient.ambient_rays is the rule's ray part):
        per hit pixel n_rays (4, 8 or 16) fixed hemisphere rays leave the voxel face the camera ray entered
        by; each one that finds nothing within `radius` (world units, inf: unbounded) adds the sky's colour
        of its direction, and the mean times the albedo times `ambient` (three numbers in [0, 4], None: off,
        the default) is added to the pixel.  variant (0..7) turns the direction table; RenderProgressive
        steps it per sample.  Only the colour outputs change."""
        before = self.GetAmbient()
        if ambient is None:
            check(_lib.lib().svo_set_ambient(self._ctx, None, 0, float("inf"), 0), "svo_set_ambient")
        else:
            a = (ctypes.c_float * 3)(*[float(v) for v in ambient])
            check(_lib.lib().svo_set_ambient(self._ctx, a, int(n_rays), float(radius), int(variant)), "svo_set_ambient")
        if self.GetAmbient() != before:   # another image: the accumulation restarts
            self.currentSample = 0

    def GetAmbient(self):
        """((r, g, b) ambient, n_rays, radius, variant) of the context (svo_get_ambient)."""
        a, n, r, v = (ctypes.c_float * 3)(), ctypes.c_int(), ctypes.c_float(), ctypes.c_uint32()
        check(_lib.lib().svo_get_ambient(self._ctx, a, ctypes.byref(n), ctypes.byref(r), ctypes.byref(v)), "svo_get_ambient")
        return (a[0], a[1], a[2]), n.value, r.value, v.value

    def SetLights(self, lights):
        """Point lights with shadow rays (svo_set_lights; lights.py is the rule): up to 8 lights, each
        (position, range, colour[, flags]) or a LIGHT_DTYPE record; None or an empty list: off, the default.
        A hit pixel whose entry face looks toward a light within its range, with nothing between the two
        (LIGHT_NO_SHADOW: unchecked), gets the light's colour times the albedo, the cosine and a smooth
        falloff that reaches 0 at `range`.  Only the colour outputs change."""
        from .lights import make_lights
        before = self.GetLights().tobytes()
        rec = make_lights(lights if lights is not None else [])
        check(_lib.lib().svo_set_lights(self._ctx, rec.ctypes.data if len(rec) else None, len(rec)), "svo_set_lights")
        if self.GetLights().tobytes() != before:   # another image: the accumulation restarts
            self.currentSample = 0

    def GetLights(self):
        """The context's lights (svo_get_lights): LIGHT_DTYPE [n]."""
        n = ctypes.c_int()
        out = np.zeros(_lib.MAX_LIGHTS, _lib.LIGHT_DTYPE)
        check(_lib.lib().svo_get_lights(self._ctx, out.ctypes.data, _lib.MAX_LIGHTS, ctypes.byref(n)), "svo_get_lights")
        return out[:n.value].copy()

    def SetObjects(self, objects):
        """Placed sub-SVOs of the renders (svo_set_objects; objects.py is the rule): up to 8 objects, each
        (root, scale_log2, position, rotation[, flags]) or an OBJECT_DTYPE record; None or an empty list: off,
        the default.  root: the descriptor index of a tree uploaded behind the terrain (SetSVOBuffer with an
        offset); the object's cube has side 32 * 2^scale_log2 world units, centred at position, rotated by
        the row-major rotation (world = R * object).  A pixel where an object is nearer than the terrain
        gets the object's record (world normal, object-local position and key) and colour."""
        from .objects import make_objects
        before = self.GetObjects().tobytes()
        rec = make_objects(objects if objects is not None else [])
        check(_lib.lib().svo_set_objects(self._ctx, rec.ctypes.data if len(rec) else None, len(rec)), "svo_set_objects")
        if self.GetObjects().tobytes() != before:   # another image: the accumulation restarts
            self.currentSample = 0

    def GetObjects(self):
        """The context's objects (svo_get_objects): OBJECT_DTYPE [n]."""
        n = ctypes.c_int()
        out = np.zeros(_lib.MAX_OBJECTS, _lib.OBJECT_DTYPE)
        check(_lib.lib().svo_get_objects(self._ctx, out.ctypes.data, _lib.MAX_OBJECTS, ctypes.byref(n)), "svo_get_objects")
        return out[:n.value].copy()

    def SetSkybox(self, texels, bilinear=True, clamp_v=False):
        """~ RayTracingShader.SetTexture(0, "_SkyboxTexture", SkyboxTexture) (RaytracingMaster.cs:28;
        svo_set_skybox): an equirectangular panorama for the rays that leave the scene.  texels: H x W x 4
        (or x 3) floats, finite and non-negative, row 0 = v = 0 (Unity's GetPixels order, bottom row
        first), alpha ignored; None: back to the procedural gradient (the default).  sky.sample_sky is the
        rule.  Only the miss pixels' colours (and bounce rays that miss) change."""
        before = self.GetSkybox()
        if texels is None:
            check(_lib.lib().svo_set_skybox(self._ctx, None, 0, 0, 0), "svo_set_skybox")
        else:
            t = np.asarray(texels, np.float32)
            if t.ndim != 3 or t.shape[2] not in (3, 4):
                raise ValueError(f"skybox texels must be H x W x 3 or H x W x 4, got {t.shape}")
            if t.shape[2] == 3:
                t = np.concatenate([t, np.ones(t.shape[:2] + (1,), np.float32)], axis=2)
            t = np.ascontiguousarray(t)
            flags = (_lib.SKY_BILINEAR if bilinear else 0) | (_lib.SKY_CLAMP_V if clamp_v else 0)
            check(_lib.lib().svo_set_skybox(self._ctx, t.ctypes.data, t.shape[1], t.shape[0], flags), "svo_set_skybox")
        if texels is not None or before != (0, 0, 0):   # another image: the accumulation restarts
            self.currentSample = 0

    def GetSkybox(self):
        """(width, height, flags) of the context's skybox texture (svo_get_skybox); (0, 0, 0): none."""
        w, h, fl = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint32()
        check(_lib.lib().svo_get_skybox(self._ctx, ctypes.byref(w), ctypes.byref(h), ctypes.byref(fl)), "svo_get_skybox")
        return w.value, h.value, fl.value

    def SampleSky(self, dirs):
        """The sky colour of n directions (svo_sample_sky_host; sky.sample_sky is its numpy statement):
        the texture if one is set, else the gradient.  dirs: n x 3 (or n x 4, w ignored), used as given,
        not normalised.  Returns n x 4 f32 (alpha 1)."""
        d = np.asarray(dirs, np.float32)
        d = d.reshape(-1, d.shape[-1] if d.ndim > 1 else 3)
        if d.shape[1] not in (3, 4):
            raise ValueError(f"directions must be n x 3 or n x 4, got {d.shape}")
        d4 = np.zeros((len(d), 4), np.float32)
        d4[:, :d.shape[1]] = d
        out = np.zeros((len(d), 4), np.float32)
        check(_lib.lib().svo_sample_sky_host(self._ctx, d4.ctypes.data, len(d4), out.ctypes.data), "svo_sample_sky_host")
        return out

    def sample_sky_device(self, dirs_ptr, n, rgba_ptr, stream=None):
        """Asynchronous svo_sample_sky on device buffers: dirs_ptr = n float4 (w ignored), rgba_ptr = n
        float4 (alpha 1), 16-byte aligned; rgba_ptr may be dirs_ptr."""
        check(_lib.lib().svo_sample_sky(self._ctx, dirs_ptr, int(n), rgba_ptr, stream), "svo_sample_sky")

    def set_count_beam(self, enable=True):
        """SVO_OPT_COUNT_BEAM: count_fetches_device counts the fetches of the walk the render runs
        (from the beam start) instead of the reference's walk from the cube entry."""
        self._set_option(_lib.SVO_OPT_COUNT_BEAM, enable)

    def set_kernel_timing(self, enable=True):
        """Bracket the primary-ray kernel of every launch with HIP events
        (measurement only; read with kernel_time())."""
        self._set_option(_lib.SVO_OPT_KERNEL_TIMING, enable)

    def kernel_time(self):
        """(mean primary-kernel ms, launches) over the launches timed since the last call."""
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        check(_lib.lib().svo_kernel_time(self._ctx, ctypes.byref(ms), ctypes.byref(n)), "svo_kernel_time")
        return ms.value, n.value

    def stage_time(self, stage):
        """(mean ms, launches) of a timed stage: _lib.STAGE_KERNEL or STAGE_ASSEMBLE."""
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        check(_lib.lib().svo_stage_time(self._ctx, int(stage), ctypes.byref(ms), ctypes.byref(n)), "svo_stage_time")
        return ms.value, n.value

    def stage_times(self, stage=_lib.STAGE_KERNEL, cap=1 << 16):
        """Every timed launch's duration (ms, float32 array in launch order) of a stage
        since the last read (svo_stage_times)."""
        out = np.zeros(cap, np.float32)
        n = ctypes.c_size_t()
        check(_lib.lib().svo_stage_times(self._ctx, int(stage), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                         cap, ctypes.byref(n)), "svo_stage_times")
        return out[:min(n.value, cap)].copy()

    def set_band_deal(self, owner=None):
        """Multi-device context: deal band b to member owner[b % len(owner)]
        (distributed.weighted_owner gives fewer bands to devices[0]); None =
        round-robin."""
        n = 0 if owner is None else len(owner)
        arr = (ctypes.c_uint8 * max(n, 1))(*([int(o) for o in owner] if owner else [0]))
        check(_lib.lib().svo_set_band_deal(self._ctx, n, arr if n else None), "svo_set_band_deal")

    def num_devices(self):
        n = ctypes.c_int()
        check(_lib.lib().svo_num_devices(self._ctx, ctypes.byref(n)), "svo_num_devices")
        return n.value

    def member_links(self):
        """[(device, link name)] per member: how each member's band payload reaches the
        display device (svo_get_member_link: "self", "xgmi_peer_pull" or "peer_copy")."""
        out = []
        for i in range(self.num_devices()):
            d, k = ctypes.c_int(), ctypes.c_int()
            check(_lib.lib().svo_get_member_link(self._ctx, i, ctypes.byref(d), ctypes.byref(k)),
                  "svo_get_member_link")
            out.append((d.value, _lib.LINK_NAMES.get(k.value, str(k.value))))
        return out

    def member(self, index):
        """The per-device context `index` (owned by this one) as a RaytracingMaster view."""
        c = ctypes.c_void_p()
        check(_lib.lib().svo_get_member(self._ctx, int(index), ctypes.byref(c)), "svo_get_member")
        return _MemberView(self, c)

    # ----------------------------------------------------------------- render
    def Render(self, width, height, stack_mode=STACK_HLSL, want_rgba=True, want_hits=True, out=None):
        """Blocking render into host arrays: (rgba[H, W, 4] float32, hits[H, W] svo_hit).
        out: an earlier call's (rgba, hits) to write again (a render loop's reused arrays; fresh
        arrays pay the first-touch page faults of 83 MB per 1080p frame)."""
        if out is not None:
            rgba, hits = out
            assert rgba is None or (rgba.dtype == np.float32 and rgba.size == height * width * 4 and rgba.flags.c_contiguous)
            assert hits is None or (hits.dtype == HIT_DTYPE and hits.size == height * width and hits.flags.c_contiguous)
        else:
            rgba = np.zeros((height, width, 4), np.float32) if want_rgba else None
            hits = np.zeros((height, width), HIT_DTYPE) if want_hits else None
        check(_lib.lib().svo_render(self._ctx, width, height, stack_mode,
                                    None if rgba is None else rgba.ctypes.data,
                                    None if hits is None else hits.ctypes.data), "svo_render")
        return rgba, hits

    def RenderProgressive(self, width, height, stack_mode=STACK_HLSL, want_rgba8=True, want_rgba=False):
        """OnRenderImage end to end (RaytracingMaster.cs:55-74): render a sample at
        the current camera, blend it into the plugin's device-resident accumulation
        frame with _Sample = currentSample (AddShader), then currentSample += 1.
        Returns (rgba8[H, W] uint32 display words or None, rgba[H, W, 4] float32
        accumulated frame or None); only those cross PCIe."""
        rgba8 = np.zeros((height, width), np.uint32) if want_rgba8 else None
        rgba = np.zeros((height, width, 4), np.float32) if want_rgba else None
        if getattr(self, "_accum_size", None) != (width, height):
            # a new render-target size (InitRenderTexture, RaytracingMaster.cs:76-88): the
            # plugin starts a fresh accumulation frame, so the sample count restarts too
            self._accum_size = (width, height)
            self.currentSample = 0
        check(_lib.lib().svo_render_progressive(self._ctx, width, height, stack_mode, self.currentSample,
                                                None if rgba8 is None else rgba8.ctypes.data,
                                                None if rgba is None else rgba.ctypes.data),
              "svo_render_progressive")
        self.currentSample += 1
        return rgba8, rgba

    def RenderProgressiveAsync(self, width, height, stack_mode=STACK_HLSL, copy=True, rgb=False):
        """OnRenderImage through the pipelined readback (svo_render_progressive_async):
        enqueue this sample and return the PREVIOUS frame's display pixels (rgba8[H, W]
        uint32 words, or with rgb=True uint8[H, W, 3]; None on the first call at a size or
        format).  copy=False returns a view of the plugin's pinned buffer, valid until the
        call after next."""
        if getattr(self, "_accum_size", None) != (width, height):
            self._accum_size = (width, height)
            self.currentSample = 0
        ptr = ctypes.c_void_p()
        fmt = _lib.PIXELS_RGB8 if rgb else _lib.PIXELS_RGBA8
        check(_lib.lib().svo_render_progressive_async(self._ctx, width, height, stack_mode, self.currentSample, fmt,
                                                      ctypes.byref(ptr)), "svo_render_progressive_async")
        self.currentSample += 1
        self._pin_rgb = rgb
        return self._pinned_frame(ptr, width, height, copy, rgb)

    def ProgressiveLast(self, width, height, copy=True):
        """The most recent frame of RenderProgressiveAsync (waits for its copy)."""
        ptr = ctypes.c_void_p()
        check(_lib.lib().svo_progressive_last(self._ctx, ctypes.byref(ptr)), "svo_progressive_last")
        return self._pinned_frame(ptr, width, height, copy, getattr(self, "_pin_rgb", False))

    @staticmethod
    def _pinned_frame(ptr, width, height, copy, rgb=False):
        if not ptr.value:
            return None
        if rgb:
            a = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(height, width, 3))
        else:
            a = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint32)), shape=(height, width))
        return a.copy() if copy else a

    def render_device(self, width, height, rgba_ptr=None, hits_ptr=None, stack_mode=STACK_HLSL,
                      band=None, stream=None):
        """Asynchronous render into device buffers (raw device pointers, e.g. torch
        tensor.data_ptr()), optionally only this rank's row bands."""
        b = None if band is None else ctypes.byref(make_band(band))
        check(_lib.lib().svo_render_device(self._ctx, width, height, stack_mode, b, rgba_ptr, hits_ptr, stream),
              "svo_render_device")

    def render_frame(self, width, height, hits=None, rgba=None, rgba8=None, compact=None, position=None,
                     voxel=None, layout=LAYOUT_BAND, stack_mode=STACK_HLSL, band=None, stream=None, rgb8=None,
                     hitmask=None):
        """Asynchronous render of every requested output (device pointers).
        layout LAYOUT_BAND: buffers hold only `band`'s rows; LAYOUT_FRAME: full-frame
        buffers.  A multi-device context renders the whole frame (band None) onto
        devices[0]."""
        # band: a (rows, rank, count[, owner]) tuple or a prebuilt _lib.SvoBand (per-frame callers
        # build it once: the owner table costs host time on every call otherwise)
        b = None if band is None else ctypes.byref(band if isinstance(band, _lib.SvoBand) else make_band(band))
        f = _frame(hits, rgba, rgba8, compact, position, voxel, layout, rgb8, hitmask)
        check(_lib.lib().svo_render_frame(self._ctx, width, height, stack_mode, b, ctypes.byref(f), stream),
              "svo_render_frame")

    def render_samples(self, width, height, offsets, first_sample, accum, rgba8=None, rgb8=None, layout=LAYOUT_BAND,
                       stack_mode=STACK_HLSL, band=None, stream=None):
        """Samples in flight (svo_render_samples): trace len(offsets) jittered samples
        (offsets: [S, 2] pixel offsets, S <= 8) in one launch and blend them in order into
        the device RGBA32F frame `accum` as _Sample = first_sample + k; rgba8 / rgb8 (device
        pointers, nullable): the blended frame's display words / 3-byte RGB."""
        off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 2)
        b = None if band is None else ctypes.byref(band if isinstance(band, _lib.SvoBand) else make_band(band))
        check(_lib.lib().svo_render_samples(self._ctx, width, height, stack_mode, b, len(off),
                                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(first_sample),
                                            accum, rgba8, rgb8, layout, stream), "svo_render_samples")

    def assemble_frame(self, width, height, parts, part_format, band_rows=None, hits=None, rgba=None, rgba8=None,
                       compact=None, skip_part=-1, stream=None, owner=None, deal=None):
        """Rebuild a frame (full-frame device buffers) from band parts: parts[m] = the
        device pointer of rank m's band payload (compact records or RGBA8 words).
        The deal: band_rows-row bands, round-robin, or owner[b % len(owner)] = the
        part holding band b (weighted deal)."""
        # parts may be a prebuilt ctypes array and deal a prebuilt _lib.SvoBand (per-frame callers)
        arr = parts if isinstance(parts, ctypes.Array) else (ctypes.c_void_p * len(parts))(*[p if p else None for p in parts])
        f = _frame(hits, rgba, rgba8, compact, None, None, LAYOUT_FRAME)
        rows = self.band_rows if band_rows is None else band_rows
        if deal is None:
            deal = make_band((rows, 0, len(parts)) if owner is None else (rows, 0, len(parts), owner))
        check(_lib.lib().svo_assemble_frame(self._ctx, width, height, ctypes.byref(deal), len(parts), arr,
                                            part_format, skip_part, ctypes.byref(f), stream),
              "svo_assemble_frame")

    def pack_hits(self, width, height, band, rgb8, part, stream=None):
        """Sparse band payload (svo_rt.h layout): `part` (device pointer, capacity
        _lib.sparse_part_bytes) starts with the band's hit masks
        (render_frame(hitmask=part)); write the tile offsets and the hit count
        behind them and pack the RGB of the hit pixels from the band's dense
        `rgb8` after that."""
        band = band if band is not None else (self.band_rows, 0, 1)
        b = ctypes.byref(band if isinstance(band, _lib.SvoBand) else make_band(band))
        check(_lib.lib().svo_pack_hits(self._ctx, width, height, b, rgb8, part, stream), "svo_pack_hits")

    # ------------------------------------------------------------ ray queries
    @staticmethod
    def _query_flags(ordered, raw):
        return (_lib.QUERY_ORDERED if ordered else 0) | (_lib.QUERY_RAW_DIRECTIONS if raw else 0)

    def TraceRays(self, origins, dirs=None, t_max=None, stack_mode=STACK_HLSL, ordered=False, raw=False,
                  want_position=False, want_voxel=False, lod=None):
        """Trace a batch of world-space rays through the SVO (svo_trace_rays_host; the reference's
        CPU-side SVO.Trace(Ray), Interfaces.cs:6-15): picking, line of sight, secondary rays.
        origins, dirs: [n, 3] (a direction is used as given, not normalised), or origins an
        array of svo_ray records (query.make_rays) and dirs None.  t_max: scalar or [n], the
        world-space parameter limit (None: no limit).  Each ray is classified and its small
        direction components clamped before it is traced (query.sanitize_rays; raw=True:
        no clamp).  ordered=True traces the rays sorted by octant and entry point: the same
        results (measured slower with its sort included).  lod=(ray_size_coef,
        ray_size_bias): level-of-detail termination for every ray of the batch (svo_trace_rays_lod_host;
        the context's own pair, SetLod, is not involved).  Blocking.  Returns the hit records
        (HIT_DTYPE [n]; t / 64 = the ray parameter of the hit; flag 0x10: invalid ray), or
        (hits, position [n, 4] or None, voxel keys [n] or None) when either is asked for."""
        from .query import make_rays
        if dirs is None:
            rays = np.ascontiguousarray(origins, _lib.RAY_DTYPE).reshape(-1)
            if t_max is not None:
                rays = rays.copy()
                rays["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), (len(rays),))
        else:
            rays = make_rays(origins, dirs, np.inf if t_max is None else t_max)
        n = len(rays)
        hits = np.zeros(n, HIT_DTYPE)
        pos = np.zeros((n, 4), np.float32) if want_position else None
        vox = np.zeros(n, np.uint64) if want_voxel else None
        outs = (hits.ctypes.data, None if pos is None else pos.ctypes.data, None if vox is None else vox.ctypes.data)
        flags = self._query_flags(ordered, raw)
        if lod is None:
            check(_lib.lib().svo_trace_rays_host(self._ctx, rays.ctypes.data, n, stack_mode, flags, *outs),
                  "svo_trace_rays_host")
        else:
            check(_lib.lib().svo_trace_rays_lod_host(self._ctx, rays.ctypes.data, n, stack_mode, flags, float(lod[0]),
                                                     float(lod[1]), *outs), "svo_trace_rays_lod_host")
        return (hits, pos, vox) if (want_position or want_voxel) else hits

    def trace_rays_device(self, rays_ptr, n, hits=None, position=None, voxel=None, hitmask=None,
                          stack_mode=STACK_HLSL, ordered=False, raw=False, stream=None, lod=None):
        """Asynchronous ray query on device buffers (svo_trace_rays): rays_ptr = n svo_ray
        records (32 bytes each, 16-byte aligned); hits (n x 24 bytes), position (n float4),
        voxel (n uint64) and hitmask (ceil(n / 64) uint64) are raw device pointers, each
        nullable, and are fully written.  lod=(ray_size_coef, ray_size_bias): svo_trace_rays_lod."""
        out = _lib.SvoQueryOut(hits, position, voxel, hitmask)
        flags = self._query_flags(ordered, raw)
        if lod is None:
            check(_lib.lib().svo_trace_rays(self._ctx, rays_ptr, int(n), stack_mode, flags, ctypes.byref(out), stream),
                  "svo_trace_rays")
        else:
            check(_lib.lib().svo_trace_rays_lod(self._ctx, rays_ptr, int(n), stack_mode, flags, float(lod[0]), float(lod[1]),
                                                ctypes.byref(out), stream), "svo_trace_rays_lod")

    def BounceRays(self, rays, hits, voxel, raw=False):
        """From a traced batch to the next one (svo_bounce_rays_host; reflection.bounce_rays is its
        numpy statement): rays (svo_ray records), their hit records and voxel keys as TraceRays
        returned them; raw: whether the batch was traced with raw=True.  Returns the bounce rays
        (RAY_DTYPE [n]): a dead ray (zero direction, invalid to TraceRays) where there was no hit."""
        rays, hits, voxel = batch_arrays(rays, hits, voxel)
        out = np.zeros(len(rays), _lib.RAY_DTYPE)
        check(_lib.lib().svo_bounce_rays_host(self._ctx, rays.ctypes.data, len(rays), self._query_flags(False, raw),
                                              hits.ctypes.data, voxel.ctypes.data, out.ctypes.data),
              "svo_bounce_rays_host")
        return out

    def bounce_rays_device(self, rays_ptr, n, hits, voxel, out, raw=False, stream=None):
        """Asynchronous svo_bounce_rays on device buffers: rays_ptr / out = n svo_ray records
        (16-byte aligned; out may be rays_ptr), hits (n x 24 bytes) and voxel (n uint64) the
        results of the batch's trace."""
        check(_lib.lib().svo_bounce_rays(self._ctx, rays_ptr, int(n), self._query_flags(False, raw), hits, voxel, out,
                                         stream), "svo_bounce_rays")

    def AmbientRays(self, rays, hits, voxel, n_rays=4, radius=float("inf"), variant=0, raw=False):
        """The ambient rays of a traced batch (svo_ambient_rays_host; ambient.ambient_rays is its numpy
        statement): rays, their hit records and voxel keys as TraceRays returned them; raw: whether the
        batch was traced with raw=True.  Returns RAY_DTYPE [n * n_rays], entry i * n_rays + k = ray k of
        rays[i]: dead rays (zero direction, invalid to TraceRays) where there was no hit."""
        rays, hits, voxel = batch_arrays(rays, hits, voxel)
        out = np.zeros(len(rays) * max(int(n_rays), 0), _lib.RAY_DTYPE)
        check(_lib.lib().svo_ambient_rays_host(self._ctx, rays.ctypes.data, len(rays), self._query_flags(False, raw),
                                               hits.ctypes.data, voxel.ctypes.data, int(n_rays), float(radius),
                                               int(variant), out.ctypes.data), "svo_ambient_rays_host")
        return out

    def ambient_rays_device(self, rays_ptr, n, hits, voxel, out, n_rays=4, radius=float("inf"), variant=0, raw=False,
                            stream=None):
        """Asynchronous svo_ambient_rays on device buffers: rays_ptr = n svo_ray records, out = n * n_rays
        (16-byte aligned, no overlap with the inputs), hits (n x 24 bytes) and voxel (n uint64) the
        results of the batch's trace."""
        check(_lib.lib().svo_ambient_rays(self._ctx, rays_ptr, int(n), self._query_flags(False, raw), hits, voxel,
                                          int(n_rays), float(radius), int(variant), out, stream), "svo_ambient_rays")

    def LightRays(self, rays, hits, voxel, lights, raw=False):
        """The shadow rays of a traced batch toward each light (svo_light_rays_host; lights.light_rays is its
        numpy statement): rays, their hit records and voxel keys as TraceRays returned them; raw: whether the
        batch was traced with raw=True.  Returns RAY_DTYPE [n * n_lights], entry i * n_lights + j = the ray of
        rays[i] toward lights[j] with t_max 1 (the light itself): a dead ray where there was no hit, or the
        light lies behind the entry face or out of range."""
        from .lights import make_lights
        rays, hits, voxel = batch_arrays(rays, hits, voxel)
        rec = make_lights(lights)
        out = np.zeros(len(rays) * len(rec), _lib.RAY_DTYPE)
        check(_lib.lib().svo_light_rays_host(self._ctx, rays.ctypes.data, len(rays), self._query_flags(False, raw),
                                             hits.ctypes.data, voxel.ctypes.data, rec.ctypes.data, len(rec),
                                             out.ctypes.data), "svo_light_rays_host")
        return out

    def light_rays_device(self, rays_ptr, n, hits, voxel, out, lights, raw=False, stream=None):
        """Asynchronous svo_light_rays on device buffers: rays_ptr = n svo_ray records, out = n * n_lights
        (16-byte aligned, no overlap with the inputs), hits (n x 24 bytes) and voxel (n uint64) the results
        of the batch's trace; lights: host records (the call copies them before it returns)."""
        from .lights import make_lights
        rec = make_lights(lights)
        check(_lib.lib().svo_light_rays(self._ctx, rays_ptr, int(n), self._query_flags(False, raw), hits, voxel,
                                        rec.ctypes.data, len(rec), out, stream), "svo_light_rays")

    def ObjectRays(self, rays, obj):
        """A batch of world rays in an object's frame (svo_object_rays_host; objects.object_rays is its numpy
        statement): rays RAY_DTYPE [n], obj one object (make_objects' forms).  Returns RAY_DTYPE [n]: {o',
        t_max, d', 0} before the small-direction clamp, a dead ray where the world ray is invalid."""
        from .objects import make_objects
        rays = np.ascontiguousarray(rays, _lib.RAY_DTYPE).reshape(-1)
        rec = make_objects(obj if isinstance(obj, (list, np.ndarray)) else [obj])
        if len(rec) != 1:
            raise ValueError(f"one object expected, {len(rec)} given")
        out = np.zeros(len(rays), _lib.RAY_DTYPE)
        check(_lib.lib().svo_object_rays_host(self._ctx, rays.ctypes.data, len(rays), 0, rec.ctypes.data,
                                              out.ctypes.data), "svo_object_rays_host")
        return out

    def object_rays_device(self, rays_ptr, n, out, obj, stream=None):
        """Asynchronous svo_object_rays on device buffers: rays_ptr / out = n svo_ray records (16-byte
        aligned; out may be rays_ptr); obj: one host record (the call copies it before it returns)."""
        from .objects import make_objects
        rec = make_objects(obj if isinstance(obj, (list, np.ndarray)) else [obj])
        check(_lib.lib().svo_object_rays(self._ctx, rays_ptr, int(n), 0, rec.ctypes.data, out, stream), "svo_object_rays")

    def TraceScene(self, rays, objects=(), stack_mode=STACK_HLSL, raw=False, terrain=True, want_position=False,
                   want_voxel=False):
        """Trace a batch of world rays through the terrain (root 0) and placed objects (svo_trace_scene_host;
        objects.py is the rule): rays RAY_DTYPE [n], objects up to 8 (make_objects' forms; the context's own
        list, SetObjects, is not involved).  terrain=False: SVO_SCENE_NO_TERRAIN.  Blocking.  Returns (hits,
        object_id) or (hits, object_id, position or None, voxel or None): the nearest hit per ray with its
        normal in world space, t / 64 the world ray's parameter, position and voxel key object-local, parent
        the absolute pool index; object_id int32 [n]: -1 a miss, 0 the terrain, j + 1 object j."""
        from .objects import make_objects
        rays = np.ascontiguousarray(rays, _lib.RAY_DTYPE).reshape(-1)
        rec = make_objects(objects if objects is not None else [])
        n = len(rays)
        hits = np.zeros(n, HIT_DTYPE)
        ids = np.zeros(n, np.int32)
        pos = np.zeros((n, 4), np.float32) if want_position else None
        vox = np.zeros(n, np.uint64) if want_voxel else None
        flags = self._query_flags(False, raw) | (0 if terrain else _lib.SCENE_NO_TERRAIN)
        check(_lib.lib().svo_trace_scene_host(self._ctx, rays.ctypes.data, n, stack_mode, flags,
                                              rec.ctypes.data if len(rec) else None, len(rec), hits.ctypes.data,
                                              None if pos is None else pos.ctypes.data,
                                              None if vox is None else vox.ctypes.data, ids.ctypes.data),
              "svo_trace_scene_host")
        return (hits, ids, pos, vox) if (want_position or want_voxel) else (hits, ids)

    def trace_scene_device(self, rays_ptr, n, objects=(), hits=None, position=None, voxel=None, hitmask=None,
                           object_id=None, stack_mode=STACK_HLSL, raw=False, terrain=True, stream=None):
        """Asynchronous svo_trace_scene on device buffers: trace_rays_device's buffers plus object_id (n int32,
        nullable); objects: host records (the call copies them before it returns)."""
        from .objects import make_objects
        rec = make_objects(objects if objects is not None else [])
        out = _lib.SvoQueryOut(hits, position, voxel, hitmask)
        flags = self._query_flags(False, raw) | (0 if terrain else _lib.SCENE_NO_TERRAIN)
        check(_lib.lib().svo_trace_scene(self._ctx, rays_ptr, int(n), stack_mode, flags,
                                         rec.ctypes.data if len(rec) else None, len(rec), ctypes.byref(out), object_id,
                                         stream), "svo_trace_scene")

    def SceneLightRays(self, rays, hits, voxel, object_id, objects, lights, raw=False):
        """The world-space shadow rays of a scene query's hits toward each light (svo_scene_light_rays_host;
        scene_light.scene_light_rays is its numpy statement): rays as given to TraceScene, its hit records,
        voxel keys and object ids, and the objects it was traced with; raw: whether it was traced with
        raw=True.  Returns RAY_DTYPE [n * n_lights], entry i * n_lights + j = the ray of hit i toward lights[j]
        with t_max 1 (the light itself): a dead ray where there was no hit, or the light lies behind the
        entered face or out of range."""
        from .lights import make_lights
        from .objects import make_objects
        rays, hits, voxel = batch_arrays(rays, hits, voxel)
        ids = np.ascontiguousarray(object_id, np.int32).reshape(-1)
        if len(ids) != len(rays):
            raise ValueError(f"{len(rays)} rays, {len(ids)} object ids")
        obs = make_objects(objects if objects is not None else [])
        rec = make_lights(lights)
        out = np.zeros(len(rays) * len(rec), _lib.RAY_DTYPE)
        check(_lib.lib().svo_scene_light_rays_host(self._ctx, rays.ctypes.data, len(rays), self._query_flags(False, raw),
                                                   hits.ctypes.data, voxel.ctypes.data, ids.ctypes.data,
                                                   obs.ctypes.data if len(obs) else None, len(obs), rec.ctypes.data,
                                                   len(rec), out.ctypes.data), "svo_scene_light_rays_host")
        return out

    def scene_light_rays_device(self, rays_ptr, n, hits, voxel, object_id, out, objects, lights, raw=False, stream=None):
        """Asynchronous svo_scene_light_rays on device buffers: rays_ptr = n svo_ray records, out = n * n_lights
        (16-byte aligned, no overlap with the inputs), hits (n x 24 bytes), voxel (n uint64) and object_id (n
        int32) the results of the batch's trace_scene_device; objects, lights: host records (the call copies
        them before it returns)."""
        from .lights import make_lights
        from .objects import make_objects
        obs = make_objects(objects if objects is not None else [])
        rec = make_lights(lights)
        check(_lib.lib().svo_scene_light_rays(self._ctx, rays_ptr, int(n), self._query_flags(False, raw), hits, voxel,
                                              object_id, obs.ctypes.data if len(obs) else None, len(obs),
                                              rec.ctypes.data, len(rec), out, stream), "svo_scene_light_rays")

    # --------------------------------------------------------- volume queries
    def OverlapVolumes(self, shapes, root=0, max_contacts=0, any_hit=False, max_visits=0, coarse_level=0):
        """Which voxels do these volumes touch (svo_overlap_volumes_host; overlap.overlap_model is its Python
        statement)?  shapes: svo_shape records (overlap.make_boxes / make_spheres), world space, or the frame of
        the tree at `root` (0: the terrain; a placed object: overlap.object_spheres).  max_contacts: K in
        0..32 contact records per shape; any_hit: stop at the first touched voxel; max_visits: the walk's budget
        of descriptor fetches (0: 65536) -- one lane of a wave walks one shape, so one huge volume holds its
        wave that long; coarse_level: report the voxels of that level instead of descending further.  Blocking.
        Returns the summaries (OVERLAP_DTYPE [n]: count, visits, flags -- bit 0 touches, 1 budget, 2 overflow,
        0x10 invalid shape), or (summaries, contacts [n, K] CONTACT_DTYPE) with max_contacts > 0."""
        shapes = np.ascontiguousarray(shapes, _lib.SHAPE_DTYPE).reshape(-1)
        n = len(shapes)
        prm = _lib.overlap_params(root, max_contacts, any_hit, max_visits, coarse_level)
        summary = np.zeros(n, _lib.OVERLAP_DTYPE)
        contacts = np.zeros((n, int(max_contacts)), _lib.CONTACT_DTYPE) if max_contacts else None
        check(_lib.lib().svo_overlap_volumes_host(self._ctx, shapes.ctypes.data, n, ctypes.byref(prm), summary.ctypes.data,
                                                  None if contacts is None else contacts.ctypes.data),
              "svo_overlap_volumes_host")
        return summary if contacts is None else (summary, contacts)

    def overlap_volumes_device(self, shapes_ptr, n, summary=None, contacts=None, hitmask=None, root=0, max_contacts=0,
                               any_hit=False, max_visits=0, coarse_level=0, stream=None):
        """Asynchronous svo_overlap_volumes on device buffers: shapes_ptr = n svo_shape records (32 bytes each,
        16-byte aligned); summary (n x 16 bytes), contacts (n x max_contacts x 16 bytes) and hitmask
        (ceil(n / 64) uint64) are raw device pointers, each nullable, and are fully written."""
        prm = _lib.overlap_params(root, max_contacts, any_hit, max_visits, coarse_level)
        out = _lib.SvoOverlapOut(summary, contacts, hitmask)
        check(_lib.lib().svo_overlap_volumes(self._ctx, shapes_ptr, int(n), ctypes.byref(prm), ctypes.byref(out), stream),
              "svo_overlap_volumes")

    # --------------------------------------------------------- closest voxels
    def ClosestVoxels(self, queries, root=0, unbounded=False, max_visits=0, coarse_level=0, contacts=False):
        """How far is each point from the surface, and where is the closest point on it (svo_closest_voxels_host;
        closest.closest_model is its Python statement)?  queries: svo_shape spheres (closest.make_queries: the
        point and a search radius), world space, or the frame of the tree at `root` (0: the terrain; a placed
        object: closest.object_queries).  unbounded: ignore the radius; max_visits: the walk's budget of
        descriptor fetches (0: 65536) -- a walk it ends returns the best so far; coarse_level: the voxels of
        that level count instead of what lies below.  Blocking.  Returns the answers (CLOSEST_DTYPE [n]: point,
        d2 -- squared, the caller takes the root --, parent, meta, visits, flags: bit 0 found, 1 budget,
        2 overflow, 0x10 invalid query), or (answers, contacts [n] CONTACT_DTYPE) with contacts=True."""
        queries = np.ascontiguousarray(queries, _lib.SHAPE_DTYPE).reshape(-1)
        n = len(queries)
        prm = _lib.closest_params(root, unbounded, max_visits, coarse_level)
        nearest = np.zeros(n, _lib.CLOSEST_DTYPE)
        found = np.zeros(n, _lib.CONTACT_DTYPE) if contacts else None
        check(_lib.lib().svo_closest_voxels_host(self._ctx, queries.ctypes.data, n, ctypes.byref(prm), nearest.ctypes.data,
                                                 None if found is None else found.ctypes.data),
              "svo_closest_voxels_host")
        return nearest if found is None else (nearest, found)

    def closest_voxels_device(self, queries_ptr, n, nearest=None, contacts=None, hitmask=None, root=0, unbounded=False,
                              max_visits=0, coarse_level=0, stream=None):
        """Asynchronous svo_closest_voxels on device buffers: queries_ptr = n svo_shape records (32 bytes each,
        16-byte aligned); nearest (n x 32 bytes), contacts (n x 16 bytes) and hitmask (ceil(n / 64) uint64) are
        raw device pointers, each nullable, and are fully written."""
        prm = _lib.closest_params(root, unbounded, max_visits, coarse_level)
        out = _lib.SvoClosestOut(nearest, contacts, hitmask)
        check(_lib.lib().svo_closest_voxels(self._ctx, queries_ptr, int(n), ctypes.byref(prm), ctypes.byref(out), stream),
              "svo_closest_voxels")

    def beam_starts_device(self, width, height, starts_ptr, band=None, stream=None):
        """svo_beam_starts: every primary ray's beam start (SVO-space t, -inf: the cube entry) into a
        device float buffer of the band's pixels (diagnostics)."""
        b = None if band is None else ctypes.byref(make_band(band))
        check(_lib.lib().svo_beam_starts(self._ctx, width, height, b, starts_ptr, stream), "svo_beam_starts")

    def count_fetches_device(self, width, height, fetch_ptr, stack_mode=STACK_HLSL, band=None, stream=None):
        b = None if band is None else ctypes.byref(make_band(band))
        check(_lib.lib().svo_count_fetches(self._ctx, width, height, stack_mode, b, fetch_ptr, stream),
              "svo_count_fetches")

    def accumulate_device(self, accum_ptr, sample_ptr, n_px, sample=None, stream=None):
        """Blend one RGBA32F sample frame into the accumulation frame (device
        pointers) with _Sample = `sample` (default: currentSample, which then
        advances like _currentSample++ after the Blit)."""
        n = self.currentSample if sample is None else int(sample)
        check(_lib.lib().svo_accumulate(self._ctx, accum_ptr, sample_ptr, int(n_px), n, stream), "svo_accumulate")
        if sample is None:
            self.currentSample += 1

    def forget_stream(self, stream):
        """svo_forget_stream: the caller is about to destroy `stream` (a hipStream_t handle)."""
        check(_lib.lib().svo_forget_stream(self._ctx, stream), "svo_forget_stream")

    def synchronize(self):
        check(_lib.lib().svo_synchronize(self._ctx), "svo_synchronize")

    def info(self):
        n = ctypes.c_size_t()
        d = ctypes.c_int()
        dev = ctypes.c_int()
        check(_lib.lib().svo_get_info(self._ctx, ctypes.byref(n), ctypes.byref(d), ctypes.byref(dev)),
              "svo_get_info")
        return {"n_nodes": n.value, "depth": d.value, "device": dev.value}

    def close(self):
        if self._ctx:
            _lib.lib().svo_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _MemberView(RaytracingMaster):
    """One device of a multi-device context: queries and device renders on that
    device alone (not destroyed on its own)."""

    def __init__(self, owner, ctx):   # noqa: D107 -- no svo_create: the group owns the context
        self._owner = owner
        self._ctx = ctx
        self._options = owner._options
        self._config = dict(owner._config)
        self.currentSample = 0
        self._c2w = None
        self.devices = None
        self.band_rows = owner.band_rows
        self.device = self.info()["device"]

    def close(self):
        self._ctx = ctypes.c_void_p()


def band_rows(height, band):
    """Global row indices owned by `band` = (band_rows, band_rank, band_count) (round-robin)
    or (band_rows, band_rank, band_count, owner) (band b belongs to owner[b % len(owner)]),
    in order."""
    rows, rank, count = band[:3]
    ys = np.arange(height)
    if len(band) == 3:
        return ys[(ys // rows) % count == rank]
    owner = np.asarray(band[3], np.int64)
    return ys[owner[(ys // rows) % len(owner)] == rank]


__all__ = ["RaytracingMaster", "SVOData", "SvoError", "STACK_HLSL", "STACK_EXACT", "HIT_DTYPE", "band_rows"]
