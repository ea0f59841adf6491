"""Builder row: NaiveCreator restatement.

Pinned by: the reference's Text dump (the CompressSVOAux layout reproduces its
4,977-descriptor topology exactly) and the digest of the reference's 3D
OpenSimplex lookup table.  The GPU leaf classification is checked against the
same sampler evaluated on the host."""
import json
import os

import numpy as np
import pytest

from raytracingtest_amd import native_builder as nb
from raytracingtest_amd.svo_data import SVOData
from raytracingtest_amd.builder import (build_from_leaves, build_menger, encode_raw_normal16, menger_solid,
                                        surface_leaves)
from tests.conftest import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def _built():
    from raytracingtest_amd import build
    build.build()


def test_opensimplex_table_matches_reference_digest():
    ref = json.load(open(os.path.join(GOLDEN, "opensimplex3d_table.json")))
    digest, n = nb.table_digest(nb.opensimplex_table())
    assert n == ref["n_hashes"] == 72
    assert digest == ref["sha256"]


def test_layout_reproduces_text_dump_topology(text_svo):
    leaves = text_svo.leaf_voxels()
    nrm = np.tile(np.float32([0, 1, 0]), (len(leaves), 1))
    ref_lo, ref_first = text_svo.masks_and_first()
    for svo in (build_from_leaves(6, leaves[:, 3:6], nrm), nb.build_from_leaves(6, leaves[:, 3:6], nrm)):
        lo, first = svo.masks_and_first()
        assert len(svo) == 4977
        assert np.array_equal(lo, ref_lo)
        has = (lo & 0xFF) != 0
        assert np.array_equal(first[has], ref_first[has])


@pytest.mark.parametrize("depth,n", [(1, 3), (3, 60), (5, 2000), (7, 20000), (9, 60000)])
def test_native_and_numpy_builders_identical(depth, n):
    rng = np.random.default_rng(depth)
    xyz = np.unique(rng.integers(0, 1 << depth, (n, 3)), axis=0)
    nrm = rng.normal(size=(len(xyz), 3)).astype(np.float32)
    a = build_from_leaves(depth, xyz, nrm)
    b = nb.build_from_leaves(depth, xyz, nrm)
    assert a.format == b.format
    assert np.array_equal(a.to_v2(), b.to_v2())
    assert np.array_equal(a.attachments, b.attachments)
    assert a.depth() == depth


def test_empty_and_single_leaf():
    e = nb.build_from_leaves(4, np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.float32))
    assert len(e) == 1 and e.childDescriptors[0] == 0
    one = nb.build_from_leaves(3, [[1, 2, 3]], [[0, 0, 1]])
    assert one.depth() == 3 and len(one) == 3


def test_menger_depth8_needs_wide_pointers():
    svo = build_menger(8)
    assert svo.format == 2 and svo.max_relative_pointer() > 0xFFFF
    assert svo.depth() == 8


def test_normal_code_roundtrip(oracle_mod):
    rng = np.random.default_rng(5)
    v = rng.normal(size=(500, 3)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    codes = encode_raw_normal16(v)
    for n, c in zip(v, codes):
        d = oracle_mod.decode_normal(int(c)).astype(np.float64)
        d /= np.linalg.norm(d)
        assert np.dot(d, n) > 0.95


def test_samplers_on_host():
    rng = np.random.default_rng(0)
    p = rng.uniform(1, 2, (20000, 3)).astype(np.float32)
    s = nb.eval_sampler(nb.SIMPLEX, p)
    assert np.all(np.abs(s) <= 1.0) and np.std(s) > 0.05
    c = nb.eval_sampler(nb.CUSTOM1, p)
    np.testing.assert_array_equal(c, nb.eval_sampler(nb.CUSTOM1, p))   # deterministic
    assert np.all(np.abs(c - (p[:, 1] - 1.5)) <= 0.65 + 1e-6)
    np.testing.assert_array_equal(nb.eval_sampler(nb.FLAT_GROUND, p), np.float32(0.5) - p[:, 1])


def _host_surface(sampler, max_level):
    """Independent host classification: sample every leaf centre (+halo) with the
    host sampler, IsEdge by 6-neighbour air test (NaiveCreator.cs:56,121-130)."""
    d = max_level - 1
    n = 1 << d
    size = np.float32(2.0 ** -d)
    c = (np.float32(1) + (np.arange(-1, n + 1, dtype=np.float32) + np.float32(0.5)) * size).astype(np.float32)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    v = nb.eval_sampler(sampler, np.stack([X, Y, Z], -1).reshape(-1, 3)).reshape(X.shape)
    solid = v <= 0
    air = v > 0
    core = solid[1:-1, 1:-1, 1:-1]
    edge = np.zeros_like(core)
    for ax in range(3):
        for s in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(s, s + n)
            edge |= air[tuple(sl)]
    return np.argwhere(core & edge)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,max_level", [(4, 5), (4, 7), (2, 6), (3, 7)])
def test_gpu_classification_matches_host(sampler, max_level):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    codes, nrm = nb.surface_leaves(sampler, max_level)
    host = _host_surface(sampler, max_level)
    from raytracingtest_amd.builder import morton
    assert np.array_equal(np.sort(morton(host)), codes)
    np.testing.assert_array_equal(nrm, _host_normals(sampler, max_level, host))


def _host_normals(sampler, max_level, host):
    """-Normalize(finite differences) (NaiveCreator.cs:58-63) of the leaves `host` (integer xyz),
    recomputed with the host sampler, in Morton order."""
    from raytracingtest_amd.builder import morton, normalize_unity
    d = max_level - 1
    size = np.float32(2.0 ** -d)
    xyz = host[np.argsort(morton(host))].astype(np.float32)
    p = (np.float32(1) + xyz * size + size / np.float32(2)).astype(np.float32)
    h = np.float32(0.001)
    s0 = nb.eval_sampler(sampler, p)
    diffs = []
    for ax in range(3):
        q = p.copy()
        q[:, ax] = (q[:, ax] - h).astype(np.float32)
        diffs.append((nb.eval_sampler(sampler, q) - s0).astype(np.float32))
    return -normalize_unity(np.stack(diffs, 1))


@pytest.fixture(scope="module")
def depth10_surface():
    """The benchmark grid's leaf pass (Custom1, max_level 11, 1024^3) twice: with the default limits
    (slabs of 508 + 508 + 8 leaf planes, seams at z = 508 and z = 1016) and with a 2 GiB byte-grid
    budget (one slab of 1026^3 cells, 1.08 GB).  (codes, normals, report) of each."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return {"default": nb.surface_leaves(nb.CUSTOM1, 11, report=True),
            "one_slab": nb.surface_leaves(nb.CUSTOM1, 11, limits={"cell_bytes": 2 << 30}, report=True)}


@pytest.mark.gpu
def test_gpu_depth10_three_slabs_equal_one_slab(depth10_surface):
    """The benchmark pool's own seams: three slabs and one slab give the same leaves and normals,
    bit for bit.  No host model of 1026^3 samples: tests/test_builder_limits.py ties one slab to
    the host model at 64^3, this ties three slabs to one at the planes the benchmark crosses."""
    codes3, nrm3, rep3 = depth10_surface["default"]
    codes1, nrm1, rep1 = depth10_surface["one_slab"]
    assert nb.slab_rows(11) == 508 and nb.slab_rows(11, {"cell_bytes": 2 << 30}) == 1024
    assert (rep3["slabs"], rep3["slab_rows"]) == (3, 508)
    assert (rep1["slabs"], rep1["slab_rows"]) == (1, 1024)
    assert rep3["relaunches"] == 0 and rep1["relaunches"] == 0   # 4 n^2 leaves hold either
    assert len(codes3) > 1_000_000
    assert np.array_equal(codes3, codes1)
    assert nrm3.tobytes() == nrm1.tobytes()


@pytest.mark.gpu
def test_gpu_build_depth10_custom1(depth10_surface):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    svo = nb.build_sampler_svo(nb.CUSTOM1, 11)
    assert svo.depth() == 10
    assert svo.n_leaves > 1_000_000
    lo, first = svo.masks_and_first()
    assert lo[0] & 0xFF00   # root has children
    codes = depth10_surface["default"][0]
    assert svo.n_leaves == len(codes)
    assert np.all(codes[1:] > codes[:-1])   # strictly increasing: sorted, no leaf twice


def test_python_sampler_matches_native_host_sampler():
    """oracle/naive_creator.py's independent OpenSimplex + samplers agree bit for
    bit with the builder's (incl. grid points where the hash comparisons tie)."""
    from oracle import naive_creator as nc
    rng = np.random.default_rng(0)
    g = (1 + (np.arange(16) + 0.5) / 16).astype(np.float32)
    pts = np.concatenate([rng.uniform(1, 2, (600, 3)).astype(np.float32),
                          np.array([[a, b, c] for a in g[:5] for b in g[:5] for c in g[:5]], np.float32)])
    for kind in (nb.SIMPLEX, nb.CUSTOM1, nb.FLAT_GROUND, nb.ROTATED_CUBOID):
        f = nc.sampler(kind)
        py = np.array([f(*q) for q in pts], np.float32)
        assert np.array_equal(py.view(np.uint32), nb.eval_sampler(kind, pts).view(np.uint32)), kind


def test_python_naive_creator_layout_matches_native():
    """The object-recursive NaiveCreator restatement and the native layout pass
    agree on descriptors and attachments for the same surface leaves."""
    from oracle import naive_creator as nc
    desc, att = nc.create(nb.CUSTOM1, 5)
    ref = SVOData(childDescriptors=desc, attachments=att)
    leaves = ref.leaf_voxels()
    # leaf normals are not stored in the pool: rebuild them from the Python tree
    root = nc.Node(nc.v3(1, 1, 1), 1, 1, False)
    nc.build_tree(root, 1, nc.sampler(nb.CUSTOM1), 5)
    xyz, nrm = [], []

    def walk(node):
        if node is None:
            return
        if node.leaf:
            xyz.append(np.round((node.position - 1) * 16).astype(np.int64))
            nrm.append(node.normal)
            return
        for c in node.children:
            walk(c)
    walk(root)
    got = nb.build_from_leaves(4, np.array(xyz), np.array(nrm, np.float32))
    assert len(leaves) == len(xyz)
    assert np.array_equal(got.childDescriptors, ref.childDescriptors)
    assert np.array_equal(got.attachments, ref.attachments)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,max_level", [(4, 3), (4, 5), (4, 6), (2, 5), (0, 4), (3, 4), (3, 6)])
def test_gpu_builder_matches_python_naive_creator(kind, max_level):
    """End to end: GPU classification + native layout == the pure-Python
    NaiveCreator restatement (descriptors and attachments bit for bit)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import naive_creator as nc
    desc, att = nc.create(kind, max_level)
    got = nb.build_sampler_svo(kind, max_level)
    assert got.format == 1
    assert np.array_equal(got.childDescriptors, desc)
    assert np.array_equal(got.attachments, att)


def test_rotated_cuboid_sampler():
    """SampleFunctions.functions[3] (SampleFunctions.cs:35-38,54-68): the restated
    Matrix4x4.Rotate(Quaternion.Euler(45, 45, 45)) is a rotation (rows orthonormal
    to float accuracy, determinant 1) and the native sampler is the rotated
    0.6-radius cube: inside at the centre, outside at the corners of [1, 2]^3, and
    at the cube's own rotated corner direction the surface lies at 0.6 * sqrt(3)."""
    from oracle import naive_creator as nc
    m = np.array(nc.unity_rotation_matrix(45, 45, 45), np.float64)
    np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-6)
    assert abs(np.linalg.det(m) - 1) < 1e-6
    pts = np.array([[1.5, 1.5, 1.5], [1, 1, 1], [2, 2, 2], [1, 2, 1]], np.float32)
    v = nb.eval_sampler(nb.ROTATED_CUBOID, pts)
    assert v[0] == np.float32(-0.6) and np.all(v[1:] > 0)
    # a point on the ray through the cube's rotated corner: world = R^T (corner) / 2 + 1.5
    corner = m.T @ np.array([1.0, 1.0, 1.0]) / np.sqrt(3)
    for t, sign in ((0.6 * np.sqrt(3) * 0.99, -1), (0.6 * np.sqrt(3) * 1.01, 1)):
        q = (corner * t / 2 + 1.5).astype(np.float32)[None]
        assert np.sign(nb.eval_sampler(nb.ROTATED_CUBOID, q)[0]) == sign
