// RaytracingMasterNative.cs -- Unity-side drop-in for Assets/Scripts/SVO/GPU/RaytracingMaster.cs
// that drives the MI355X plugin (libsvo_rt.so, include/svo_rt.h) through P/Invoke instead of
// ComputeShader.Dispatch.  NOT compiled in this repository (no C# toolchain in the build image);
// it is the binding a Unity maintainer adds next to the reference script (see INTEGRATION.md).
using System;
using System.Runtime.InteropServices;
using UnityEngine;
using static SvoNative;   // SvoHit in the MonoBehaviour's Raycast signatures

public static class SvoNative {
    const string Lib = "svo_rt";        // libsvo_rt.so in Assets/Plugins/x86_64
    const string Builder = "svo_build"; // libsvo_build.so: the native NaiveCreator (include/svo_build.h)
    public const int StackHlsl = 0, StackExact = 1;

    [StructLayout(LayoutKind.Sequential)]
    public struct SvoHit { public uint parent; public byte hitIdx; public byte hitScale; public ushort flags;
                           public float t, nx, ny, nz; }                          // 24 bytes == svo_hit

    [DllImport(Lib)] public static extern int svo_create(int device, UIntPtr capacityNodes, out IntPtr ctx);
    [DllImport(Lib)] public static extern int svo_create_multi(int[] devices, int numDevices, UIntPtr capacityNodes,
                                                               int bandRows, out IntPtr ctx);
    [DllImport(Lib)] public static extern int svo_set_buffer(IntPtr ctx, int[] desc, UIntPtr nDesc,
                                                             uint[] att, UIntPtr nAtt, UIntPtr dstOffset);
    // wide node format (svo_rt.h): first_child_abs << 32 | valid << 8 | nonleaf -- any pool the builder makes,
    // straight from the builder's native arrays (no managed copy)
    [DllImport(Lib)] public static extern int svo_set_buffer_v2(IntPtr ctx, IntPtr nodes, UIntPtr nNodes,
                                                                IntPtr att, UIntPtr nAtt, UIntPtr dstOffset);
    [DllImport(Lib)] public static extern int svo_get_info(IntPtr ctx, out UIntPtr nNodes, out int maxDepth,
                                                           out int device);
    [DllImport(Lib)] public static extern int svo_set_camera(IntPtr ctx, float[] c2w, float[] invProj,
                                                             float pxOffX, float pxOffY, float[] light);
    [DllImport(Lib)] public static extern int svo_render(IntPtr ctx, int width, int height, int stackMode,
                                                         float[] rgbaOut, [Out] SvoHit[] hitsOut);
    [DllImport(Lib)] public static extern int svo_render_progressive(IntPtr ctx, int width, int height, int stackMode,
                                                                     uint sample, [Out] uint[] rgba8Out,
                                                                     [Out] float[] rgbaOut);
    // pipelined readback: returns the previous frame's RGBA8 words in plugin-owned pinned memory
    // (valid until the call after next), the D2H of this frame overlapping the next render
    public const int PixelsRgba8 = 0, PixelsRgb8 = 1;   // TextureFormat.RGBA32 / RGB24
    [DllImport(Lib)] public static extern int svo_render_progressive_async(IntPtr ctx, int width, int height,
                                                                           int stackMode, uint sample, int pixelFormat,
                                                                           out IntPtr frame);
    [DllImport(Lib)] public static extern int svo_destroy(IntPtr ctx);
    [DllImport(Lib)] public static extern IntPtr svo_last_error();

    // svo_config (include/svo_rt.h, ABI 10): the render policy, versioned by size -- field order and
    // types exactly the header's (132 bytes; tests/test_boundary.py checks the C layout)
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoConfig {
        public uint size, version;
        public int tileOrder, xcdStrips, issuePriority, orderEvery, moveEvery, moveSpread, relayout, fetchAll,
                   loopForm;
        public float latRatio;
        public int segments;
        public uint segTableLatency, segTableIssue, segTableThin;
        public float segRatio, segThinRatio;
        public int segCap, segMinChain, segMove, segJitter, segAll;
        public uint segScramble;
        public int beam, beamBack, shadowForm, shadowOrder, readback, hostCopyThreads, sparsePayload, peerCopy;
        public int beamBackHeld;   // config version 2
    }
    [DllImport(Lib)] public static extern int svo_get_config(IntPtr ctx, ref SvoConfig cfg);
    [DllImport(Lib)] public static extern int svo_set_config(IntPtr ctx, ref SvoConfig cfg);

    // Ray queries (svo_trace_rays, include/svo_rt.h): the GPU counterpart of the reference's CPU-side
    // SVO.Trace(UnityEngine.Ray) (Interfaces.cs:6-15).  svo_ray: 32 bytes, the header's field order.
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoRay {
        public float originX, originY, originZ;   // world space
        public float tMax;                        // ray-parameter limit (+inf: none)
        public float dirX, dirY, dirZ;            // used as given, not normalised
        public uint reserved;                     // 0
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoQueryOut { public IntPtr hits, position, voxel, hitmask; }   // device pointers
    public const uint QueryOrdered = 1, QueryRawDirections = 2;
    public const ushort HitInvalidRay = 0x10;     // SvoHit.flags bit 4
    [DllImport(Lib)] public static extern int svo_trace_rays(IntPtr ctx, IntPtr dRays, UIntPtr nRays, int stackMode,
                                                             uint flags, ref SvoQueryOut output, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_trace_rays_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr nRays,
                                                                  int stackMode, uint flags, [Out] SvoHit[] hits,
                                                                  [Out] float[] position, [Out] ulong[] voxel);
    // Level of detail (svo_rt.h): the primary rays' pair of the context, and queries with a pair of their own
    [DllImport(Lib)] public static extern int svo_set_lod(IntPtr ctx, float raySizeCoef, float raySizeBias);
    [DllImport(Lib)] public static extern int svo_get_lod(IntPtr ctx, out float raySizeCoef, out float raySizeBias);
    [DllImport(Lib)] public static extern int svo_trace_rays_lod(IntPtr ctx, IntPtr dRays, UIntPtr nRays, int stackMode,
                                                                 uint flags, float raySizeCoef, float raySizeBias,
                                                                 ref SvoQueryOut output, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_trace_rays_lod_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr nRays,
                                                                      int stackMode, uint flags, float raySizeCoef,
                                                                      float raySizeBias, [Out] SvoHit[] hits,
                                                                      [Out] float[] position, [Out] ulong[] voxel);
    // Specular reflection (svo_rt.h): the bounce-ray building block of the ray queries, and the renders' setting
    [DllImport(Lib)] public static extern int svo_bounce_rays(IntPtr ctx, IntPtr dRays, UIntPtr n, uint flags, IntPtr dHits,
                                                              IntPtr dVoxel, IntPtr dRaysOut, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_bounce_rays_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr n, uint flags,
                                                                   [In] SvoHit[] hits, [In] ulong[] voxel,
                                                                   [Out] SvoRay[] raysOut);
    [DllImport(Lib)] public static extern int svo_set_reflection(IntPtr ctx, [In] float[] specular, int maxBounces);
    [DllImport(Lib)] public static extern int svo_get_reflection(IntPtr ctx, [Out] float[] specular, out int maxBounces);
    // Ambient (svo_rt.h): sky light with ambient occlusion -- the renders' setting and the ray queries' building block
    public const int AmbientMaxRays = 16;
    [DllImport(Lib)] public static extern int svo_set_ambient(IntPtr ctx, [In] float[] ambient, int nRays, float radius,
                                                              uint variant);
    [DllImport(Lib)] public static extern int svo_get_ambient(IntPtr ctx, [Out] float[] ambient, out int nRays,
                                                              out float radius, out uint variant);
    [DllImport(Lib)] public static extern int svo_ambient_rays(IntPtr ctx, IntPtr dRays, UIntPtr n, uint flags, IntPtr dHits,
                                                               IntPtr dVoxel, int nRays, float radius, uint variant,
                                                               IntPtr dRaysOut, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_ambient_rays_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr n, uint flags,
                                                                    [In] SvoHit[] hits, [In] ulong[] voxel, int nRays,
                                                                    float radius, uint variant, [Out] SvoRay[] raysOut);
    // Lights (svo_rt.h): up to 8 point lights with shadow rays -- the renders' setting and the ray queries' building block
    public const int MaxLights = 8;
    public const uint LightNoShadow = 1;
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoLight {          // svo_light, 32 bytes
        public Vector3 position;      // world space, |component| <= 2^20
        public float range;           // world units, in (0, 2^20]
        public Vector3 colour;        // colour x intensity, each in [0, 65536]
        public uint flags;            // LightNoShadow
    }
    [DllImport(Lib)] public static extern int svo_set_lights(IntPtr ctx, [In] SvoLight[] lights, int nLights);
    [DllImport(Lib)] public static extern int svo_get_lights(IntPtr ctx, [Out] SvoLight[] lights, int cap, out int nLights);
    [DllImport(Lib)] public static extern int svo_light_rays(IntPtr ctx, IntPtr dRays, UIntPtr n, uint flags, IntPtr dHits,
                                                             IntPtr dVoxel, [In] SvoLight[] lights, int nLights,
                                                             IntPtr dRaysOut, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_light_rays_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr n, uint flags,
                                                                  [In] SvoHit[] hits, [In] ulong[] voxel,
                                                                  [In] SvoLight[] lights, int nLights, [Out] SvoRay[] raysOut);
    // Objects (svo_rt.h): sub-SVOs of the pool placed in the world -- the renders' list and the scene query
    public const int MaxObjects = 8;
    public const uint SceneNoTerrain = 4;
    [Serializable]
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoObject {         // svo_object, 64 bytes
        public uint root;             // descriptor index of the object's root in the pool
        public int scaleLog2;         // k in [-8, 8]: the cube has side 32 * 2^k world units
        public uint flags;            // 0
        public Vector3 position;      // world position of the cube's centre, |component| <= 2^20
        public float r00, r01, r02, r10, r11, r12, r20, r21, r22;   // row-major R, world = R * object
        public uint reserved;         // 0
    }
    [DllImport(Lib)] public static extern int svo_set_objects(IntPtr ctx, [In] SvoObject[] objects, int nObjects);
    [DllImport(Lib)] public static extern int svo_get_objects(IntPtr ctx, [Out] SvoObject[] objects, int cap, out int nObjects);
    [DllImport(Lib)] public static extern int svo_object_rays(IntPtr ctx, IntPtr dRays, UIntPtr n, uint flags,
                                                              [In] ref SvoObject obj, IntPtr dRaysOut, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_object_rays_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr n, uint flags,
                                                                   [In] ref SvoObject obj, [Out] SvoRay[] raysOut);
    [DllImport(Lib)] public static extern int svo_trace_scene(IntPtr ctx, IntPtr dRays, UIntPtr n, int stackMode, uint flags,
                                                              [In] SvoObject[] objects, int nObjects, IntPtr queryOut,
                                                              IntPtr dObject, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_trace_scene_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr n, int stackMode,
                                                                   uint flags, [In] SvoObject[] objects, int nObjects,
                                                                   [Out] SvoHit[] hits, [Out] Vector4[] position,
                                                                   [Out] ulong[] voxel, [Out] int[] objectId);
    // Render options (svo_rt.h svo_set_options): the directional light's shadow rays, and the shadow and light passes
    // that know the placed objects
    public const uint OptShadowRays = 1, OptSceneShadows = 8;
    [DllImport(Lib)] public static extern int svo_set_options(IntPtr ctx, uint options);
    // Objects in light (svo_rt.h): svo_light_rays for the results of svo_trace_scene, world-space shadow rays
    [DllImport(Lib)] public static extern int svo_scene_light_rays(IntPtr ctx, IntPtr dRays, UIntPtr n, uint flags, IntPtr dHits,
                                                                   IntPtr dVoxel, IntPtr dObject, [In] SvoObject[] objects,
                                                                   int nObjects, [In] SvoLight[] lights, int nLights,
                                                                   IntPtr dRaysOut, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_scene_light_rays_host(IntPtr ctx, [In] SvoRay[] rays, UIntPtr n, uint flags,
                                                                        [In] SvoHit[] hits, [In] ulong[] voxel,
                                                                        [In] int[] objectId, [In] SvoObject[] objects,
                                                                        int nObjects, [In] SvoLight[] lights, int nLights,
                                                                        [Out] SvoRay[] raysOut);
    // Skybox (svo_rt.h): the reference's _SkyboxTexture for rays that leave the scene, and its rule for ray queries
    public const uint SkyBilinear = 1, SkyClampV = 2;
    [DllImport(Lib)] public static extern int svo_set_skybox(IntPtr ctx, [In] Color[] rgba, int width, int height, uint flags);
    [DllImport(Lib)] public static extern int svo_get_skybox(IntPtr ctx, out int width, out int height, out uint flags);
    [DllImport(Lib)] public static extern int svo_sample_sky(IntPtr ctx, IntPtr dDirs, UIntPtr n, IntPtr dRgba, IntPtr stream);
    [DllImport(Lib)] public static extern int svo_sample_sky_host(IntPtr ctx, [In] Vector4[] dirs, UIntPtr n, [Out] Color[] rgba);
    // Volume queries (svo_rt.h): which voxels a world-space box or sphere touches.  svo_shape: 32 bytes, the
    // header's field order; the frame is the tree's own world convention, the cube [-16, 16]^3.
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoShape {
        public float pX, pY, pZ;                  // box: the low corner; sphere: the centre
        public uint kind;                         // ShapeBox, ShapeSphere
        public float qX, qY, qZ;                  // box: the high corner; sphere: qX the radius, qY = qZ = 0
        public uint reserved;                     // 0
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoContact {                    // == svo_contact, 16 bytes
        public uint parent;                       // descriptor holding the voxel; 0xFFFFFFFF: unused entry
        public uint meta;                         // hit_idx | hit_scale << 8
        public ulong key;                         // the voxel key of a ray hit
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoOverlap {                    // == svo_overlap, 16 bytes
        public uint count, visits, flags, reserved;   // flags: bit0 touches, bit1 budget, bit2 overflow, 0x10 invalid shape
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoOverlapParams {              // == svo_overlap_params, versioned by size
        public uint size, flags, root, maxContacts, maxVisits, coarseLevel;
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoOverlapOut { public IntPtr summary, contacts, hitmask; }   // device pointers
    public const uint ShapeBox = 0, ShapeSphere = 1, OverlapAny = 1;
    public const int OverlapMaxContacts = 32;
    [DllImport(Lib)] public static extern int svo_overlap_volumes(IntPtr ctx, IntPtr dShapes, UIntPtr n,
                                                                  ref SvoOverlapParams prm, ref SvoOverlapOut output,
                                                                  IntPtr stream);
    [DllImport(Lib)] public static extern int svo_overlap_volumes_host(IntPtr ctx, [In] SvoShape[] shapes, UIntPtr n,
                                                                       ref SvoOverlapParams prm, [Out] SvoOverlap[] summary,
                                                                       [Out] SvoContact[] contacts);
    // Closest voxels (svo_rt.h): the nearest voxel to a point, its squared distance and the closest point on it.
    // A query is an SvoShape of kind ShapeSphere: the point and a search radius (ClosestUnbounded ignores it).
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoClosest {                    // == svo_closest, 32 bytes
        public float pointX, pointY, pointZ;      // closest point on the voxel's closed box; not found: 0, 0, 0
        public float d2;                          // squared distance; not found: +inf
        public uint parent, meta, visits, flags;  // flags: bit0 found, bit1 budget, bit2 overflow, 0x10 invalid query
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoClosestParams {              // == svo_closest_params, versioned by size
        public uint size, flags, root, maxVisits, coarseLevel;
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvoClosestOut { public IntPtr nearest, contacts, hitmask; }   // device pointers
    public const uint ClosestUnbounded = 1;
    [DllImport(Lib)] public static extern int svo_closest_voxels(IntPtr ctx, IntPtr dQueries, UIntPtr n,
                                                                 ref SvoClosestParams prm, ref SvoClosestOut output,
                                                                 IntPtr stream);
    [DllImport(Lib)] public static extern int svo_closest_voxels_host(IntPtr ctx, [In] SvoShape[] queries, UIntPtr n,
                                                                      ref SvoClosestParams prm, [Out] SvoClosest[] nearest,
                                                                      [Out] SvoContact[] contacts);

    [StructLayout(LayoutKind.Sequential)]
    public struct SvobResult {   // == svob_result
        public UIntPtr nNodes; public int depth; public int v1Ok;
        public IntPtr descriptors, nodes, attachments; public UIntPtr nLeaves;
    }
    [DllImport(Builder)] public static extern int svob_build_sampler(int device, int sampler, int maxLevel,
                                                                     out SvobResult result);
    // Meshes (include/svo_build.h "Triangle meshes"): positions in the cube's unit frame [0,1]^3
    public const uint MeshFlipWinding = 1;   // SVOB_MESH_FLIP_WINDING: Unity's front faces are clockwise
    [StructLayout(LayoutKind.Sequential)]
    public struct SvobMesh {     // == svob_mesh, 48 bytes, versioned by size
        public uint size, flags;
        public IntPtr positions; public UIntPtr nVertices;    // float xyz per vertex
        public IntPtr indices; public UIntPtr nTriangles;     // 3 uint per triangle
        public IntPtr colors;                                 // float rgb per vertex, or zero
    }
    [StructLayout(LayoutKind.Sequential)]
    public struct SvobMeshStats {   // == svob_mesh_stats, 40 bytes
        public uint size, reserved;
        public ulong degenerate, outside, candidates, overlaps;
    }
    // limits and report: IntPtr.Zero for the defaults / no report
    [DllImport(Builder)] public static extern int svob_build_mesh(int device, ref SvobMesh mesh, int maxLevel, IntPtr limits,
                                                                  IntPtr report, ref SvobMeshStats stats, out SvobResult result);
    [DllImport(Builder)] public static extern void svob_free(ref SvobResult result);
    [DllImport(Builder)] public static extern IntPtr svob_last_error();

    public static void Check(int rc, string what) {
        if (rc != 0) throw new InvalidOperationException(what + ": " + Marshal.PtrToStringAnsi(svo_last_error()));
    }
    public static void CheckBuild(int rc, string what) {
        if (rc != 0) throw new InvalidOperationException(what + ": " + Marshal.PtrToStringAnsi(svob_last_error()));
    }

    // The HLSL float2 stack (NVIDIASVO.compute:98) rounds parent indices above 2^24 nodes
    // (SURVEY.md Appendix A): such pools (C4, C5) trace with the exact stack
    public static int StackModeFor(IntPtr ctx) {
        Check(svo_get_info(ctx, out UIntPtr n, out int depth, out int device), "svo_get_info");
        // parents above 2^24 are rounded by the HLSL stack, and so is a popped t_max (2^-17 relative): pools of
        // 16 levels and more lose voxels seen from outside the cube (INTEGRATION.md "Stack mode")
        return (ulong)n > (1UL << 24) || depth >= 16 ? StackExact : StackHlsl;
    }

    // Unity Matrix4x4 is column-major in memory (m00, m10, m20, m30, m01, ...), which is the C-ABI order.
    public static float[] ToArray(Matrix4x4 m) {
        var a = new float[16];
        for (int i = 0; i < 16; i++) a[i] = m[i];   // Matrix4x4 indexer is column-major
        return a;
    }
}

public class RaytracingMasterNative : MonoBehaviour {
    public Light DirectionalLight;
    // the reference's [Range(1, 8)] (RaytracingMaster.cs:16-17) is widened: the native builder
    // makes the BASELINE pools up to 8192^3 (maxLevel 14) in seconds
    [Range(1, 14)] public int maxLevel = 5;
    public SampleFunctions.Type sampleType = SampleFunctions.Type.Custom1;
    [Range(1, 8)] public int gpus = 1;   // > 1: the frame is split in 8-row bands over GPUs 0..gpus-1

    // Render policy (svo_config): the Inspector fields a developer tunes; the defaults are the
    // library's (svo_get_config(NULL)).  None changes the image -- only where the time goes.
    [Header("Render policy (svo_config)")]
    public bool beamStarts = true;               // beam: rays start at their tile's lower bound of the hit t
    [Range(0, 8)] public int beamBack = 2;       // a new view's splat: boxes this many levels above the leaves
    [Range(-1, 8)] public int beamBackHeld = 0;  // a held view's finer re-splat (-1: beamBack)
    public bool segmentedRays = true;            // segments: heavy tiles traced as exact t-segments
    public bool costOrderedDispatch = true;      // tile_order: heaviest tiles dispatched first
    [Range(1, 32)] public int moveEvery = 4;     // while the camera moves, rebuild the order every k-th frame
    // Level of detail (svo_set_lod; NOT render policy: it changes the image): a voxel smaller than this many
    // pixels ends the walk like a leaf.  0 = off.  Not supported together with shadow rays.
    [Range(0, 16)] public float lodPixels = 0;
    float _lodPixelsSet = 0;
    // Specular reflection (svo_set_reflection; it changes the image): the reference's `specular` (hard-coded 0,
    // RaytraceCompute.compute:97-104) per channel in [0, 1] and the bounce rays per pixel; zero = off.  Not
    // supported together with shadow rays, lodPixels or gpus > 1.
    public Vector3 specular;
    [Range(0,7)] public int maxBounces;
    Vector3 _specularSet;
    int _maxBouncesSet = 0;
    // Ambient (svo_set_ambient; it changes the image; the reference has none): per hit pixel ambientRays (0 = off,
    // 4, 8 or 16) hemisphere rays about the voxel face; each one that finds nothing within ambientRadius world
    // units (0 = unbounded) adds the sky of its direction, and the mean times the albedo times `ambient` (per
    // channel in [0, 4]) is added.  The accumulation turns the direction table per sample.  Not supported together
    // with specular, lodPixels or gpus > 1.
    public Vector3 ambient;
    [Range(0, 16)] public int ambientRays;
    public float ambientRadius = 0;
    Vector3 _ambientSet;
    int _ambientRaysSet = 0;
    float _ambientRadiusSet = 0;
    // Skybox (svo_set_skybox; it changes the image): the reference's SkyboxTexture (RaytracingMaster.cs:6), an
    // equirectangular panorama (readable, at most 8192 x 8192), uploaded once when the context is created as the
    // reference binds it once in Awake (:28).  None: the procedural gradient.  Not supported with gpus > 1.
    public Texture2D SkyboxTexture;
    public bool skyboxBilinear = true;           // the texture's filterMode Bilinear (false: Point)
    public bool skyboxClampV;                    // wrapModeV Clamp (false: Repeat, Unity's import default)
    public enum ShadowForm { Fused = 0, TilePass = 1, CompactedList = 2 }
    public ShadowForm shadowForm = ShadowForm.Fused;
    // Shadow rays toward the directional light (SVO_OPT_SHADOW_RAYS; it changes the image), and beside it the
    // switch that lets shadow rays and point lights see the placed objects (SVO_OPT_SCENE_SHADOWS): objects then
    // cast and receive shadows, every shadow ray may walk up to eight more cubes, and without it a render with
    // placed objects refuses shadow rays and lights.
    public bool shadowRays;
    public bool sceneShadows;

    IntPtr _ctx;
    Camera _camera;
    Texture2D _frame;
    uint[] _rgba8;
    uint _currentSample = 0;   // RaytracingMaster.cs:12
    int _stackMode = SvoNative.StackHlsl;   // chosen from the uploaded pool (SvoNative.StackModeFor)

    void Awake() {
        _camera = GetComponent<Camera>();
        InitializeSVOBuffer();
    }

    // RaytracingMaster.cs:44-53: a moved camera restarts the accumulation; key R rebuilds the SVO
    void Update() {
        if (transform.hasChanged) {
            _currentSample = 0;
            transform.hasChanged = false;
        }
        if (Input.GetKeyDown(KeyCode.R)) SetSVOBuffer();
    }

    // SVODriver.UpdateRaycast's query (SVODriver.cs:74-87) on the GPU: the first voxel along the ray within
    // maxDistance (direction normalised here, so hit.t / 64 is the world distance).  Exactly axis-aligned
    // directions work: the plugin restores the small-direction clamp the reference commented out.
    public bool Raycast(Vector3 origin, Vector3 direction, float maxDistance, out SvoHit hit, out Vector3 point) {
        var rays = new[] { new Ray(origin, direction) };
        SvoHit[] hits;
        Vector3[] points;
        Raycast(rays, maxDistance, out hits, out points);
        hit = hits[0];
        point = points[0];
        return (hit.flags & 1) != 0;
    }

    // Batch overload: one svo_trace_rays_host call for all rays; returns the number of hits.  ordered: trace in
    // the order of the rays' octant and entry point (the same results; measured slower, DESIGN.md 3.2b).
    public int Raycast(Ray[] rays, float maxDistance, out SvoHit[] hits, out Vector3[] points, bool ordered = false) {
        var list = new SvoNative.SvoRay[rays.Length];
        for (int i = 0; i < rays.Length; i++) {
            Vector3 o = rays[i].origin, d = rays[i].direction;   // UnityEngine.Ray keeps a unit direction
            list[i] = new SvoNative.SvoRay { originX = o.x, originY = o.y, originZ = o.z, tMax = maxDistance,
                                             dirX = d.x, dirY = d.y, dirZ = d.z, reserved = 0 };
        }
        hits = new SvoHit[rays.Length];
        points = new Vector3[rays.Length];
        if (rays.Length == 0) return 0;
        SvoNative.Check(SvoNative.svo_trace_rays_host(_ctx, list, (UIntPtr)rays.Length, _stackMode,
                                                      ordered ? SvoNative.QueryOrdered : 0u, hits, null, null),
                        "svo_trace_rays_host");
        int n = 0;
        for (int i = 0; i < rays.Length; i++) {
            if ((hits[i].flags & 1) == 0) continue;
            points[i] = rays[i].GetPoint(hits[i].t / 64.0f);   // world hit point = origin + (t / 64) dir
            n++;
        }
        return n;
    }

    // Which voxels do these volumes touch (svo_overlap_volumes_host)?  Collision broad-phase, spawn placement,
    // trigger volumes.  Shapes in world space (SvoNative.SvoShape: a box or a sphere); root 0 is the terrain.
    // maxContacts: 0..32 contact records per shape (contacts[i * maxContacts ..], Morton order; null with 0);
    // anyHit: stop at the first voxel; maxVisits: the walk's budget of descriptor fetches (0: 65536) -- one GPU
    // lane walks one shape, so keep huge volumes on a small budget or a coarseLevel.  Returns how many touch.
    public int OverlapVolumes(SvoNative.SvoShape[] shapes, out SvoNative.SvoOverlap[] summary,
                              out SvoNative.SvoContact[] contacts, uint root = 0, int maxContacts = 0, bool anyHit = false,
                              uint maxVisits = 0, uint coarseLevel = 0) {
        summary = new SvoNative.SvoOverlap[shapes.Length];
        contacts = maxContacts > 0 ? new SvoNative.SvoContact[shapes.Length * maxContacts] : null;
        if (shapes.Length == 0) return 0;
        var prm = new SvoNative.SvoOverlapParams {
            size = (uint)Marshal.SizeOf(typeof(SvoNative.SvoOverlapParams)), flags = anyHit ? SvoNative.OverlapAny : 0u,
            root = root, maxContacts = (uint)maxContacts, maxVisits = maxVisits, coarseLevel = coarseLevel };
        SvoNative.Check(SvoNative.svo_overlap_volumes_host(_ctx, shapes, (UIntPtr)shapes.Length, ref prm, summary, contacts),
                        "svo_overlap_volumes_host");
        int n = 0;
        for (int i = 0; i < summary.Length; i++)
            if ((summary[i].flags & 1) != 0) n++;
        return n;
    }

    // How far is each point from the surface, and where is the closest point on it (svo_closest_voxels_host)?
    // Depenetration, conservative advancement (step by distance - r), snap-to-surface, clearance tests.  Queries
    // in world space (SvoNative.SvoShape of kind ShapeSphere: the point, qX the search radius); root 0 is the
    // terrain.  unbounded: ignore the radius; maxVisits: the walk's budget of descriptor fetches (0: 65536) -- a
    // walk it ends answers with the best so far.  d2 is squared: take Mathf.Sqrt.  Returns how many found a voxel.
    public int ClosestVoxels(SvoNative.SvoShape[] queries, out SvoNative.SvoClosest[] nearest,
                             out SvoNative.SvoContact[] contacts, uint root = 0, bool unbounded = false,
                             uint maxVisits = 0, uint coarseLevel = 0) {
        nearest = new SvoNative.SvoClosest[queries.Length];
        contacts = new SvoNative.SvoContact[queries.Length];
        if (queries.Length == 0) return 0;
        var prm = new SvoNative.SvoClosestParams {
            size = (uint)Marshal.SizeOf(typeof(SvoNative.SvoClosestParams)),
            flags = unbounded ? SvoNative.ClosestUnbounded : 0u, root = root, maxVisits = maxVisits, coarseLevel = coarseLevel };
        SvoNative.Check(SvoNative.svo_closest_voxels_host(_ctx, queries, (UIntPtr)queries.Length, ref prm, nearest, contacts),
                        "svo_closest_voxels_host");
        int n = 0;
        for (int i = 0; i < nearest.Length; i++)
            if ((nearest[i].flags & 1) != 0) n++;
        return n;
    }

    // RaytracingMaster.cs:111-116
    public void InitializeSVOBuffer() {
        CreateContext((UIntPtr)(1073741824 / 8));
    }

    void CreateContext(UIntPtr capacity) {
        IntPtr ctx;
        if (gpus <= 1) {
            SvoNative.Check(SvoNative.svo_create(0, capacity, out ctx), "svo_create");
        } else {   // one SVO replica per GPU, bands gathered to GPU 0 over xGMI; every other call is unchanged
            var devices = new int[gpus];
            for (int i = 0; i < gpus; i++) devices[i] = i;
            SvoNative.Check(SvoNative.svo_create_multi(devices, gpus, capacity, 8, out ctx), "svo_create_multi");
        }
        _ctx = ctx;
        ApplyConfig();
        UploadSkybox();
    }

    // RaytracingMaster.cs:28.  GetPixels returns the texels row by row from the bottom row, which is the plugin's
    // row 0 = v = 0 (INTEGRATION.md "Skybox": reasoned from the API documentation, not observed).
    void UploadSkybox() {
        if (SkyboxTexture == null) return;
        uint flags = (skyboxBilinear ? SvoNative.SkyBilinear : 0u) | (skyboxClampV ? SvoNative.SkyClampV : 0u);
        SvoNative.Check(SvoNative.svo_set_skybox(_ctx, SkyboxTexture.GetPixels(), SkyboxTexture.width, SkyboxTexture.height,
                                                 flags), "svo_set_skybox");
    }

    // the Inspector fields into the context's svo_config; the other fields keep the library's values
    void ApplyConfig() {
        if (_ctx == IntPtr.Zero) return;
        var cfg = new SvoNative.SvoConfig { size = (uint)Marshal.SizeOf<SvoNative.SvoConfig>() };
        SvoNative.Check(SvoNative.svo_get_config(_ctx, ref cfg), "svo_get_config");
        cfg.beam = beamStarts ? 1 : 0;
        cfg.beamBack = beamBack;
        cfg.beamBackHeld = beamBackHeld;
        cfg.segments = segmentedRays ? 1 : 0;
        cfg.tileOrder = costOrderedDispatch ? 1 : 0;
        cfg.moveEvery = moveEvery;
        cfg.shadowForm = (int)shadowForm;
        SvoNative.Check(SvoNative.svo_set_config(_ctx, ref cfg), "svo_set_config");
        uint options = (shadowRays ? SvoNative.OptShadowRays : 0u) | (sceneShadows ? SvoNative.OptSceneShadows : 0u);
        SvoNative.Check(SvoNative.svo_set_options(_ctx, options), "svo_set_options");
    }

    void OnValidate() { ApplyConfig(); }   // an Inspector edit at run time takes effect at the next frame

    // RaytracingMaster.cs:90-109 (key R): NaiveCreator.Create(SampleFunctions.functions[sampleType], maxLevel)
    // by the native builder on GPU 0, uploaded in the wide node format -- every BASELINE pool from
    // 256^3 up has child pointers beyond the reference's 16 bits.  The pool replaces the old one (the
    // capacity is the 1 GiB of InitializeSVOBuffer; a bigger pool gets a context of its size).
    void SetSVOBuffer() {
        // SampleFunctions.functions[5] (Custom2) is null in the reference (SampleFunctions.cs:13-48):
        // its key R would throw there too; say so instead of calling the builder
        if ((int)sampleType > (int)SampleFunctions.Type.Custom1) {
            Debug.LogError("sampleType " + sampleType + " has no sampler in the reference (SampleFunctions.functions)");
            return;
        }
        SvoNative.CheckBuild(SvoNative.svob_build_sampler(0, (int)sampleType, maxLevel, out var r), "svob_build_sampler");
        try {
            ulong n = (ulong)r.nNodes;
            if (n > (ulong)(1073741824 / 8)) {   // beyond InitializeSVOBuffer's capacity
                SvoNative.svo_destroy(_ctx);
                _ctx = IntPtr.Zero;                // never left pointing at the freed context
                CreateContext((UIntPtr)n);         // assigns _ctx only once the new context exists
            }
            SvoNative.Check(SvoNative.svo_set_buffer_v2(_ctx, r.nodes, r.nNodes, r.attachments, (UIntPtr)(2 * n),
                                                        UIntPtr.Zero), "svo_set_buffer_v2");
        } finally {
            SvoNative.svob_free(ref r);
        }
        _stackMode = SvoNative.StackModeFor(_ctx);
        _currentSample = 0;
    }

    // A Unity Mesh as a pool behind the terrain: its bounds are mapped uniformly into the unit cube with a 2 %
    // margin, svob_build_mesh voxelises it on GPU 0 at maxLevel, and the pool is uploaded at node dstOffset in the
    // wide format -- place it with SetObjects (root = dstOffset).  Unity's front faces are clockwise in its
    // left-handed frame: the winding flag keeps the normals outward.  Returns the pool's node count.
    public ulong SetSVOFromMesh(Mesh mesh, int maxLevel, ulong dstOffset) {
        Vector3[] verts = mesh.vertices;
        int[] tris = mesh.triangles;
        Color[] cols = mesh.colors;
        Bounds b = mesh.bounds;
        float extent = Mathf.Max(b.size.x, Mathf.Max(b.size.y, b.size.z));
        float scale = extent > 0f ? 0.96f / extent : 1f;
        var pos = new float[3 * verts.Length];
        for (int i = 0; i < verts.Length; ++i) {
            Vector3 p = (verts[i] - b.center) * scale;
            pos[3 * i] = 0.5f + p.x; pos[3 * i + 1] = 0.5f + p.y; pos[3 * i + 2] = 0.5f + p.z;
        }
        var idx = new uint[tris.Length];
        for (int i = 0; i < tris.Length; ++i) idx[i] = (uint)tris[i];
        float[] rgb = null;
        if (cols != null && cols.Length == verts.Length) {
            rgb = new float[3 * cols.Length];
            for (int i = 0; i < cols.Length; ++i) { rgb[3 * i] = cols[i].r; rgb[3 * i + 1] = cols[i].g; rgb[3 * i + 2] = cols[i].b; }
        }
        GCHandle hp = GCHandle.Alloc(pos, GCHandleType.Pinned), hi = GCHandle.Alloc(idx, GCHandleType.Pinned);
        GCHandle hc = rgb != null ? GCHandle.Alloc(rgb, GCHandleType.Pinned) : default(GCHandle);
        try {
            var m = new SvoNative.SvobMesh {
                size = (uint)Marshal.SizeOf(typeof(SvoNative.SvobMesh)), flags = SvoNative.MeshFlipWinding,
                positions = hp.AddrOfPinnedObject(), nVertices = (UIntPtr)verts.Length,
                indices = hi.AddrOfPinnedObject(), nTriangles = (UIntPtr)(tris.Length / 3),
                colors = rgb != null ? hc.AddrOfPinnedObject() : IntPtr.Zero };
            var stats = new SvoNative.SvobMeshStats { size = (uint)Marshal.SizeOf(typeof(SvoNative.SvobMeshStats)) };
            SvoNative.CheckBuild(SvoNative.svob_build_mesh(0, ref m, maxLevel, IntPtr.Zero, IntPtr.Zero, ref stats, out var r),
                                 "svob_build_mesh");
            try {
                ulong n = (ulong)r.nNodes;
                // wide nodes hold ABSOLUTE first-child indices: a pool that does not start at node 0 is rebased
                for (ulong i = 0; dstOffset != 0 && i < n; ++i) {
                    long node = Marshal.ReadInt64(r.nodes, (int)(8 * i));
                    if ((node & 0xFF) != 0) Marshal.WriteInt64(r.nodes, (int)(8 * i), node + ((long)dstOffset << 32));
                }
                SvoNative.Check(SvoNative.svo_set_buffer_v2(_ctx, r.nodes, r.nNodes, r.attachments, (UIntPtr)(2 * n),
                                                            (UIntPtr)dstOffset), "svo_set_buffer_v2");
                _stackMode = SvoNative.StackModeFor(_ctx);
                _currentSample = 0;
                return n;
            } finally {
                SvoNative.svob_free(ref r);
            }
        } finally {
            hp.Free(); hi.Free();
            if (rgb != null) hc.Free();
        }
    }

    // RaytracingMaster.cs:118-135 (attachments land at 2*offset: the reference's offset bug is fixed)
    public void SetSVOBuffer(RT.SVOData data, int offset = 0) {
        var desc = data.childDescriptors.ToArray();
        var att = data.attachments.ToArray();
        SvoNative.Check(SvoNative.svo_set_buffer(_ctx, desc, (UIntPtr)desc.Length, att, (UIntPtr)att.Length,
                                                 (UIntPtr)offset), "svo_set_buffer");
        _stackMode = SvoNative.StackModeFor(_ctx);
    }

    // RaytracingMaster.cs:32-41 + 55-74: the sample is rendered, blended into the plugin's
    // device-resident accumulation frame with _Sample = _currentSample (AddShader.shader:44-47),
    // and only the accumulated display frame (RGBA8, 4 B/px) crosses PCIe -- into the plugin's
    // pinned buffer, on a copy stream, while the next frame renders: the call returns the
    // PREVIOUS frame's words, which LoadRawTextureData copies straight from that pointer (no
    // managed array).  One frame of display latency; pipelined = false uses the blocking call.
    public bool pipelined = true;

    void OnRenderImage(RenderTexture source, RenderTexture destination) {
        Vector3 l = DirectionalLight.transform.forward;
        SvoNative.Check(SvoNative.svo_set_camera(_ctx, SvoNative.ToArray(_camera.cameraToWorldMatrix),
                                                 SvoNative.ToArray(_camera.projectionMatrix.inverse),
                                                 UnityEngine.Random.value, UnityEngine.Random.value,
                                                 new[] { l.x, l.y, l.z, DirectionalLight.intensity }), "svo_set_camera");
        int w = Screen.width, h = Screen.height;
        // ray_size_coef: the footprint of lodPixels pixels at the frame's centre per unit t of a unit ray
        SvoNative.Check(SvoNative.svo_set_lod(_ctx, lodPixels * 2f * Mathf.Abs(_camera.projectionMatrix.inverse[1, 1]) / h, 0f),
                        "svo_set_lod");
        if (lodPixels != _lodPixelsSet) { _lodPixelsSet = lodPixels; _currentSample = 0; }   // another image: a fresh accumulation
        SvoNative.Check(SvoNative.svo_set_reflection(_ctx, new[] { specular.x, specular.y, specular.z }, maxBounces),
                        "svo_set_reflection");
        if (specular != _specularSet || maxBounces != _maxBouncesSet) {   // another image as well
            _specularSet = specular; _maxBouncesSet = maxBounces; _currentSample = 0;
        }
        SvoNative.Check(SvoNative.svo_set_ambient(_ctx, new[] { ambient.x, ambient.y, ambient.z }, ambientRays,
                                                  ambientRadius > 0f ? ambientRadius : float.PositiveInfinity, 0u),
                        "svo_set_ambient");
        if (ambient != _ambientSet || ambientRays != _ambientRaysSet || ambientRadius != _ambientRadiusSet) {   // and here
            _ambientSet = ambient; _ambientRaysSet = ambientRays; _ambientRadiusSet = ambientRadius; _currentSample = 0;
        }
        // the pipelined path moves 3-byte pixels (RGB24: a quarter fewer bytes over PCIe); `pipelined`
        // is an Inspector field, so a toggle at run time recreates the texture in the other format
        TextureFormat want = pipelined ? TextureFormat.RGB24 : TextureFormat.RGBA32;
        if (_frame == null || _frame.width != w || _frame.height != h || _frame.format != want) {
            _frame = new Texture2D(w, h, want, false, true);
            _rgba8 = new uint[w * h];
            _currentSample = 0;   // a new render target: the plugin starts a fresh accumulation frame
        }
        if (pipelined) {
            SvoNative.Check(SvoNative.svo_render_progressive_async(_ctx, w, h, _stackMode, _currentSample,
                                                                   SvoNative.PixelsRgb8, out IntPtr prev),
                            "svo_render_progressive_async");
            if (prev != IntPtr.Zero) {   // NULL only on the first frame at this size
                _frame.LoadRawTextureData(prev, w * h * 3);
                _frame.Apply(false);
            }
        } else {
            SvoNative.Check(SvoNative.svo_render_progressive(_ctx, w, h, _stackMode, _currentSample, _rgba8, null),
                            "svo_render_progressive");
            _frame.SetPixelData(_rgba8, 0);
            _frame.Apply(false);
        }
        Graphics.Blit(_frame, destination);   // already accumulated: a plain copy, no AddMaterial
        _currentSample++;
    }

    // Point lights of the scene on the voxel world (svo_set_lights; it changes the image; the reference has
    // _DirectionalLight only): up to 8 Unity point lights, colour x intensity, Light.range as the range.  Call it
    // when the lights change; null or an empty array turns them off.  Not supported together with specular,
    // lodPixels, ambient or gpus > 1.
    public void SetLights(Light[] pointLights, bool shadows = true) {
        int n = pointLights == null ? 0 : Mathf.Min(pointLights.Length, SvoNative.MaxLights);
        var rec = new SvoNative.SvoLight[n];
        for (int j = 0; j < n; ++j) {
            Color c = pointLights[j].color * pointLights[j].intensity;
            rec[j].position = pointLights[j].transform.position;
            rec[j].range = pointLights[j].range;
            rec[j].colour = new Vector3(c.r, c.g, c.b);
            rec[j].flags = shadows && pointLights[j].shadows != LightShadows.None ? 0u : SvoNative.LightNoShadow;
        }
        SvoNative.Check(SvoNative.svo_set_lights(_ctx, n > 0 ? rec : null, n), "svo_set_lights");
        _currentSample = 0;   // another image: a fresh accumulation
    }

    // A voxel model placed on the voxel world (svo_set_objects): its tree was uploaded behind the terrain at
    // descriptor index `root`; the Transform gives the placement.  Serialisable, so a scene keeps its list.
    [Serializable]
    public struct PlacedObject {
        public uint root;             // where the model's tree lies in the pool
        public int scaleLog2;         // the cube's side is 32 * 2^scaleLog2 world units
        public Transform transform;   // position and rotation (its scale is not read: uniform powers of two only)
    }
    public PlacedObject[] placedObjects;

    // The placed objects of the renders (svo_set_objects; it changes the image): up to 8.  Call it whenever one
    // moves; null or an empty array turns them off.  Shadow rays and lights need sceneShadows
    // with them; not supported together with specular, lodPixels, ambient or gpus > 1.
    public void SetObjects(PlacedObject[] objects) {
        int n = objects == null ? 0 : Mathf.Min(objects.Length, SvoNative.MaxObjects);
        var rec = new SvoNative.SvoObject[n];
        for (int j = 0; j < n; ++j) {
            Matrix4x4 m = Matrix4x4.Rotate(objects[j].transform.rotation);
            rec[j].root = objects[j].root;
            rec[j].scaleLog2 = objects[j].scaleLog2;
            rec[j].position = objects[j].transform.position;
            rec[j].r00 = m.m00; rec[j].r01 = m.m01; rec[j].r02 = m.m02;
            rec[j].r10 = m.m10; rec[j].r11 = m.m11; rec[j].r12 = m.m12;
            rec[j].r20 = m.m20; rec[j].r21 = m.m21; rec[j].r22 = m.m22;
        }
        SvoNative.Check(SvoNative.svo_set_objects(_ctx, n > 0 ? rec : null, n), "svo_set_objects");
        placedObjects = objects;
        _currentSample = 0;   // another image: a fresh accumulation
    }

    void OnDestroy() {
        if (_ctx != IntPtr.Zero) SvoNative.svo_destroy(_ctx);
    }
}
