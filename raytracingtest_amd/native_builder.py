"""ctypes front-end of libsvo_build.so (include/svo_build.h): the native
restatement of NaiveCreator (Assets/Scripts/SVO/CompactSVO/NaiveCreator.cs)
with GPU leaf classification."""
import ctypes
import os

import numpy as np

from ._lib import BUILDER_PATH, SvoError, _load_torch_first
from .svo_data import SVOData

# SampleFunctions.Type (SampleFunctions.cs:4-11)
FLAT_GROUND, SPHERE, SIMPLEX, ROTATED_CUBOID, CUSTOM1 = range(5)


class _Result(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_size_t), ("depth", ctypes.c_int), ("v1_ok", ctypes.c_int),
                ("descriptors", ctypes.POINTER(ctypes.c_int32)), ("nodes", ctypes.POINTER(ctypes.c_uint64)),
                ("attachments", ctypes.POINTER(ctypes.c_uint32)), ("n_leaves", ctypes.c_size_t)]


class _Limits(ctypes.Structure):
    """svob_limits (include/svo_build.h): zero is the default of every field."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("cell_bytes", ctypes.c_uint64),
                ("list_capacity", ctypes.c_uint64), ("slab_rows", ctypes.c_int32), ("max_blocks", ctypes.c_int32),
                ("launch_candidates", ctypes.c_uint64)]


class _Report(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("slabs", ctypes.c_uint32), ("slab_rows", ctypes.c_uint32),
                ("relaunches", ctypes.c_uint32), ("normals_regrown", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("list_capacity", ctypes.c_uint64), ("overlap_launches", ctypes.c_uint32),
                ("reserved2", ctypes.c_uint32)]


class _Mesh(ctypes.Structure):
    """svob_mesh (include/svo_build.h), versioned by size."""
    _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("positions", ctypes.c_void_p),
                ("n_vertices", ctypes.c_size_t), ("indices", ctypes.c_void_p), ("n_triangles", ctypes.c_size_t),
                ("colors", ctypes.c_void_p)]


class _MeshStats(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("degenerate", ctypes.c_uint64),
                ("outside", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("overlaps", ctypes.c_uint64)]


MESH_FLIP_WINDING = 1
MESH_STATS_FIELDS = ("degenerate", "outside", "candidates", "overlaps")
LIMIT_FIELDS = ("cell_bytes", "slab_rows", "list_capacity", "max_blocks", "launch_candidates")
REPORT_FIELDS = ("slabs", "slab_rows", "relaunches", "normals_regrown", "list_capacity")
MESH_REPORT_FIELDS = REPORT_FIELDS + ("overlap_launches",)   # the mesh entries' report; the samplers leave it 0


def _limits(limits):
    """None, or a mapping with any of LIMIT_FIELDS -> a svob_limits (None: NULL, all defaults)."""
    if limits is None:
        return None
    unknown = set(limits) - set(LIMIT_FIELDS)
    if unknown:
        raise SvoError(f"unknown builder limits {sorted(unknown)}: the fields are {LIMIT_FIELDS}")
    lim = _Limits(size=ctypes.sizeof(_Limits))
    for k, v in limits.items():
        setattr(lim, k, int(v))
    return ctypes.byref(lim)


def _new_report():
    return _Report(size=ctypes.sizeof(_Report))


def _report_dict(rep, fields=REPORT_FIELDS):
    return {k: int(getattr(rep, k)) for k in fields}


_blib = None


def blib():
    global _blib
    if _blib is None:
        if not os.path.exists(BUILDER_PATH):
            raise SvoError(f"{BUILDER_PATH} is not built: run __graft_entry__.build()")
        _load_torch_first()
        L = ctypes.CDLL(BUILDER_PATH, mode=ctypes.RTLD_GLOBAL)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.svob_build_sampler.argtypes = [i, i, i, ctypes.POINTER(_Result)]
        L.svob_build_from_leaves.argtypes = [i, sz, vp, vp, vp, ctypes.POINTER(_Result)]
        L.svob_surface_leaves.argtypes = [i, i, i, ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.svob_build_sampler_ex.argtypes = [i, i, i, vp, vp, ctypes.POINTER(_Result)]
        L.svob_surface_leaves_ex.argtypes = [i, i, i, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(vp),
                                             ctypes.POINTER(vp)]
        L.svob_slab_rows.argtypes = [i, vp]
        L.svob_build_mesh.argtypes = [i, vp, i, vp, vp, vp, ctypes.POINTER(_Result)]
        L.svob_mesh_leaves.argtypes = [i, vp, i, vp, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                       ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.svob_eval_sampler.argtypes = [i, sz, vp, vp]
        L.svob_opensimplex_table.argtypes = [vp]
        L.svob_mesh_profile.argtypes = [i, vp]
        L.svob_mesh_profile.restype = i
        L.svob_free.argtypes = [ctypes.POINTER(_Result)]
        L.svob_free.restype = None
        L.svob_free_ptr.argtypes = [vp]
        L.svob_free_ptr.restype = None
        L.svob_last_error.restype = ctypes.c_char_p
        for name in ("svob_build_sampler", "svob_build_from_leaves", "svob_surface_leaves", "svob_eval_sampler",
                     "svob_opensimplex_table", "svob_build_sampler_ex", "svob_surface_leaves_ex", "svob_slab_rows",
                     "svob_build_mesh", "svob_mesh_leaves"):
            getattr(L, name).restype = i
        _blib = L
    return _blib


def _check(rc, what):
    if rc != 0:
        raise SvoError(f"{what} failed ({rc}): {blib().svob_last_error().decode(errors='replace')}")


def _to_svodata(res, prefer_v1=True):
    n = res.n_nodes
    att = np.ctypeslib.as_array(res.attachments, shape=(2 * n,)).copy()
    if prefer_v1 and res.v1_ok:
        desc = np.ctypeslib.as_array(res.descriptors, shape=(n,)).copy()
        return SVOData(childDescriptors=desc, attachments=att)
    nodes = np.ctypeslib.as_array(res.nodes, shape=(n,)).copy()
    return SVOData(nodes=nodes, attachments=att)


def slab_rows(max_level, limits=None):
    """Leaf planes per z-slab of the GPU leaf pass (svob_slab_rows; host arithmetic, no GPU)."""
    rows = blib().svob_slab_rows(int(max_level), _limits(limits))
    if rows < 1:
        _check(rows, "svob_slab_rows")
    return rows


def build_sampler_svo(sample_type, max_level, device=0, prefer_v1=True, limits=None, report=False):
    """NaiveCreator.Create(SampleFunctions.functions[sample_type], max_level).
    limits: None or a mapping with any of LIMIT_FIELDS (svob_limits; they never change the
    result).  report=True: returns (svo, dict of REPORT_FIELDS)."""
    res = _Result()
    rep = _new_report()
    _check(blib().svob_build_sampler_ex(int(device), int(sample_type), int(max_level), _limits(limits),
                                        ctypes.byref(rep), ctypes.byref(res)), "svob_build_sampler")
    try:
        data = _to_svodata(res, prefer_v1)
        data.n_leaves = int(res.n_leaves)
        return (data, _report_dict(rep)) if report else data
    finally:
        blib().svob_free(ctypes.byref(res))


def build_from_leaves(depth, xyz, normals, colors=None, prefer_v1=True):
    """CompressSVO over given surface leaves (native twin of builder.build_from_leaves)."""
    xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    col = None if colors is None else np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    res = _Result()
    _check(blib().svob_build_from_leaves(int(depth), len(xyz), xyz.ctypes.data, normals.ctypes.data,
                                         None if col is None else col.ctypes.data, ctypes.byref(res)),
           "svob_build_from_leaves")
    try:
        return _to_svodata(res, prefer_v1)
    finally:
        blib().svob_free(ctypes.byref(res))


def surface_leaves(sample_type, max_level, device=0, limits=None, report=False):
    """(Morton codes uint64[n], normals float32[n, 3]) of the surface voxels; with report=True a
    third item, the dict of REPORT_FIELDS.  limits: as build_sampler_svo."""
    n = ctypes.c_size_t()
    mp = ctypes.c_void_p()
    npp = ctypes.c_void_p()
    rep = _new_report()
    _check(blib().svob_surface_leaves_ex(int(device), int(sample_type), int(max_level), _limits(limits),
                                         ctypes.byref(rep), ctypes.byref(n), ctypes.byref(mp), ctypes.byref(npp)),
           "svob_surface_leaves")
    try:
        codes = np.ctypeslib.as_array(ctypes.cast(mp, ctypes.POINTER(ctypes.c_uint64)), shape=(n.value,)).copy() \
            if n.value else np.zeros(0, np.uint64)
        nrm = np.ctypeslib.as_array(ctypes.cast(npp, ctypes.POINTER(ctypes.c_float)), shape=(n.value, 3)).copy() \
            if n.value else np.zeros((0, 3), np.float32)
        return (codes, nrm, _report_dict(rep)) if report else (codes, nrm)
    finally:
        blib().svob_free_ptr(mp)
        blib().svob_free_ptr(npp)


def _mesh(positions, triangles, colors, flip):
    """A svob_mesh over contiguous copies of the arrays; returns (struct, the arrays it points into)."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles).reshape(-1, 3)
    if tri.size and (tri.min() < 0 or tri.max() > 0xFFFFFFFF):
        raise SvoError("triangle indices must fit uint32")
    tri = np.ascontiguousarray(tri, np.uint32)
    col = None if colors is None else np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    if col is not None and len(col) != len(pos):
        raise SvoError(f"colors holds {len(col)} rgb for {len(pos)} vertices")
    m = _Mesh(size=ctypes.sizeof(_Mesh), flags=MESH_FLIP_WINDING if flip else 0, positions=pos.ctypes.data,
              n_vertices=len(pos), indices=tri.ctypes.data, n_triangles=len(tri),
              colors=None if col is None else col.ctypes.data)
    return m, (pos, tri, col)


def _stats_dict(st):
    return {k: int(getattr(st, k)) for k in MESH_STATS_FIELDS}


def build_mesh_svo(positions, triangles, max_level, colors=None, flip=False, device=0, prefer_v1=True, limits=None,
                   report=False):
    """svob_build_mesh: an indexed triangle mesh (positions [v, 3] in the cube's unit frame [0,1]^3, triangles
    [t, 3], optional per-vertex rgb) voxelised on the GPU by the rule of voxelize.py and laid out as
    build_from_leaves does.  flip: SVOB_MESH_FLIP_WINDING.  limits: as build_sampler_svo (they never change the
    result; "launch_candidates" cuts a slab's candidates into launches of the overlap kernel).  report=True:
    returns (svo, dict of MESH_REPORT_FIELDS, dict of MESH_STATS_FIELDS)."""
    m, keep = _mesh(positions, triangles, colors, flip)
    res = _Result()
    rep = _new_report()
    st = _MeshStats(size=ctypes.sizeof(_MeshStats))
    _check(blib().svob_build_mesh(int(device), ctypes.byref(m), int(max_level), _limits(limits), ctypes.byref(rep),
                                  ctypes.byref(st), ctypes.byref(res)), "svob_build_mesh")
    del keep
    try:
        data = _to_svodata(res, prefer_v1)
        data.n_leaves = int(res.n_leaves)
        return (data, _report_dict(rep, MESH_REPORT_FIELDS), _stats_dict(st)) if report else data
    finally:
        blib().svob_free(ctypes.byref(res))


MESH_KERNELS = ("setup", "count", "scan", "overlap", "compact", "attributes")


def mesh_profile(enable):
    """svob_mesh_profile: switch the per-kernel device-event timing of this thread's mesh calls; returns the
    sums of the last timed call, {kernel: milliseconds}."""
    ms = (ctypes.c_double * len(MESH_KERNELS))()
    _check(blib().svob_mesh_profile(1 if enable else 0, ms), "svob_mesh_profile")
    return dict(zip(MESH_KERNELS, (float(v) for v in ms)))


def mesh_leaves(positions, triangles, max_level, colors=None, flip=False, device=0, limits=None, report=False):
    """svob_mesh_leaves: (Morton codes uint64[m] sorted, normals float32[m, 3], colours float32[m, 3] or None,
    owner uint32[m]) -- voxelize.voxelize's result at depth max_level - 1, from the GPU; with report=True two more
    items, the dicts of MESH_REPORT_FIELDS and MESH_STATS_FIELDS."""
    m, keep = _mesh(positions, triangles, colors, flip)
    n = ctypes.c_size_t()
    ptrs = [ctypes.c_void_p() for _ in range(4)]   # morton, normals, colours, owner
    rep = _new_report()
    st = _MeshStats(size=ctypes.sizeof(_MeshStats))
    _check(blib().svob_mesh_leaves(int(device), ctypes.byref(m), int(max_level), _limits(limits), ctypes.byref(rep),
                                   ctypes.byref(st), ctypes.byref(n), *[ctypes.byref(p) for p in ptrs]),
           "svob_mesh_leaves")
    del keep
    try:
        k = n.value

        def arr(p, ctype, shape, dtype):
            if not k:
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=shape).copy()
        codes = arr(ptrs[0], ctypes.c_uint64, (k,), np.uint64)
        nrm = arr(ptrs[1], ctypes.c_float, (k, 3), np.float32)
        col = arr(ptrs[2], ctypes.c_float, (k, 3), np.float32) if ptrs[2].value else None
        owner = arr(ptrs[3], ctypes.c_uint32, (k,), np.uint32)
        out = (codes, nrm, col, owner)
        return out + (_report_dict(rep, MESH_REPORT_FIELDS), _stats_dict(st)) if report else out
    finally:
        for p in ptrs:
            blib().svob_free_ptr(p)


def eval_sampler(sample_type, xyz):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros(len(xyz), np.float32)
    _check(blib().svob_eval_sampler(int(sample_type), len(xyz), xyz.ctypes.data, out.ctypes.data),
           "svob_eval_sampler")
    return out


def opensimplex_table():
    out = np.zeros((2048, 25), np.int8)
    _check(blib().svob_opensimplex_table(out.ctypes.data), "svob_opensimplex_table")
    return out


def table_digest(table):
    """sha256 of the canonical {hash: [count, offsets...]} listing."""
    import hashlib
    rows = []
    for h in range(2048):
        c = int(table[h, 0])
        if c:
            rows.append(f"{h}:" + ",".join(str(int(v)) for v in table[h, 1:1 + 3 * c]))
    return hashlib.sha256("\n".join(rows).encode()).hexdigest(), len(rows)
