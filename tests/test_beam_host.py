"""The host side of the beam starts (raytracingtest_amd/csrc/svo_beam.h: the splat list of a pool and the
splat's view of a camera) on a CPU, against the models of tests/beam_model.py.  tests/beam_host_driver.cpp,
a plain C++ program that includes only that header, evaluates every case below in one run; the same
program runs once more under AddressSanitizer + UndefinedBehaviorSanitizer, as a process of its own.

Splat lists are compared exactly: the same boxes in the same order (Morton at 16 bits; the order of equal
keys is free).  On every list: the boxes are pairwise disjoint, every leaf voxel lies in exactly one box,
no box is deeper than min(depth - back, 16).  The camera is compared with the float64 model built from
camera_ray's formulas."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from raytracingtest_amd.builder import build_from_leaves, build_menger
from raytracingtest_amd.camera import Camera, column_major
from tests import beam_model as bm
from tests.conftest import ROOT

GXX = shutil.which("g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
HIP_INC = "/opt/rocm/include"


# ------------------------------------------------------------------ pools
def _arrays(svo):
    lo, first = svo.masks_and_first()
    return lo.astype(np.uint32), first.astype(np.uint32)


def _random_leaf_tree(depth, seed):
    rng = np.random.default_rng(seed)
    n = 1 << depth
    k = min(400, max(1, n ** 3 // 3))
    flat = rng.choice(n ** 3, size=k, replace=False)
    xyz = np.stack([flat % n, flat // n % n, flat // (n * n)], axis=1)
    return build_from_leaves(depth, xyz, np.tile(np.array([0.0, 1.0, 0.0], np.float32), (k, 1)))


def rand_subtree(rng, depth, nodes):
    """Append a random subtree of exactly `depth` descriptor levels, leaves at every level (one branch
    goes to the bottom); a node's non-leaf children are contiguous, in ascending slot order.  Its root index."""
    root = len(nodes)
    nodes.append(0)
    valid = int(rng.integers(1, 256))
    if depth == 1:
        nodes[root] = valid << 8
        return root
    nonleaf = valid & int(rng.integers(0, 256)) or valid & -valid
    kids = [c for c in range(8) if (nonleaf >> c) & 1]
    deep = int(rng.choice(kids))
    first = len(nodes)
    nodes.extend([0] * len(kids))
    for j, c in enumerate(kids):
        sub = rand_subtree(rng, depth - 1 if c == deep else int(rng.integers(1, depth)), nodes)
        nodes[first + j] = nodes[sub]   # the reserved slot takes the subtree root's descriptor
    nodes[root] = (first << 32) | (valid << 8) | nonleaf
    return root


def _split(nodes):
    a = np.array(nodes, np.uint64)
    return (a & np.uint64(0xFFFFFFFF)).astype(np.uint32), (a >> np.uint64(32)).astype(np.uint32)


def mixed_depth_tree(seed=11, depth=6):
    nodes = []
    rand_subtree(np.random.default_rng(seed), depth, nodes)
    return _split(nodes)


def dag_pool():
    """The pool of test_gpu_frame.test_dag_pool_shared_node_at_two_depths: a shared 6-level subtree S reached
    at depth 2 (0 -> 1 -> S) and at depth 4 (0 -> 2 -> 3 -> S); the longest path has 9 levels."""
    rng = np.random.default_rng(3)
    nodes = [0, 0, 0, 0]
    s_root = rand_subtree(rng, 6, nodes)
    nodes[0] = (1 << 32) | (0x81 << 8) | 0x81
    nodes[1] = (s_root << 32) | (0x01 << 8) | 0x01
    nodes[2] = (3 << 32) | (0x80 << 8) | 0x80
    nodes[3] = (s_root << 32) | (0x40 << 8) | 0x40
    return _split(nodes)


def longest_path(lo, first, n):
    """Descriptor levels on the longest path from the root (a child index >= n: an empty descriptor, one level)."""
    memo = {}

    def dep(v):
        if v >= n:
            return 1
        if v not in memo:
            inner = int(lo[v]) & 0xFF
            kids = [int(first[v]) + bin(inner & ((1 << c) - 1)).count("1") for c in range(8) if (inner >> c) & 1]
            memo[v] = 1 + max([dep(k) for k in kids], default=0)
        return memo[v]
    return dep(0)


_POOLS = {}


def _pools(text_svo):
    """name -> (lo, first, depth, leaves as (x, y, z, level) rows); built once."""
    if _POOLS:
        return _POOLS
    out = _POOLS
    trees = {"text": text_svo, "menger3": build_menger(3, 2)}
    for d in (1, 2, 5, 9):
        trees[f"random{d}"] = _random_leaf_tree(d, 100 + d)
    for name, svo in trees.items():
        lo, first = _arrays(svo)
        lv = svo.leaf_voxels()[:, [3, 4, 5, 2]]
        mine = bm.positional_leaves(lo, first)
        assert sorted(map(tuple, lv.tolist())) == sorted(map(tuple, mine.tolist())), name   # the walk used for the DAG
        out[name] = (lo, first, svo.depth(), lv)
    lo, first = mixed_depth_tree()
    out["mixed"] = (lo, first, longest_path(lo, first, len(lo)), bm.positional_leaves(lo, first))
    lo, first = dag_pool()
    out["dag"] = (lo, first, longest_path(lo, first, len(lo)), bm.positional_leaves(lo, first))
    lo, first, depth, _ = out["random5"]
    n = len(lo) * 2 // 3                       # the last third of the nodes is not uploaded
    lo, first = lo[:n].copy(), first[:n].copy()
    out["cut"] = (lo, first, depth, bm.positional_leaves(lo, first))
    return out


def list_cases(text_svo):
    cases = []
    for name, (lo, first, depth, leaves) in _pools(text_svo).items():
        for back in sorted({0, 1, 2, depth - 1, depth, depth + 3}):
            cases.append((f"{name} back={back}", lo, first, depth, back, 1 << 23, leaves))
    lo, first, depth, leaves = _pools(text_svo)["dag"]
    cases.append(("dag budget=64", lo, first, depth, 0, 64, leaves))
    cases.append(("dag budget=1", lo, first, depth, 0, 1, leaves))
    return cases


# ------------------------------------------------------------------ cameras
def _cam_words(c2w, inv_proj):
    return np.concatenate([column_major(c2w), column_major(inv_proj)]).view(np.uint32)


def camera_cases():
    from test_gpu_beam import _cams
    cases = []
    for (w, h) in ((256, 144), (13, 3)):
        for name, cam in _cams().items():
            c2w, ip = cam.uniforms(w, h)
            cases.append((f"{name} {w}x{h}", w, h, c2w, ip, True))
    w, h = 256, 144
    c2w, ip = Camera().uniforms(w, h)
    for what, (r, c) in (("nan", (0, 3)), ("nan", (1, 1)), ("inf", (2, 3)), ("-inf", (0, 2))):
        bad = c2w.copy()
        bad[r, c] = np.float32(what)
        cases.append((f"{what} in c2w[{r}][{c}]", w, h, bad, ip, False))
    sing = ip.copy()
    sing[:, 0] = 0.0                 # no dependence on u: M's first column is zero
    cases.append(("singular inv_proj", w, h, c2w, sing, False))
    flat = ip.copy()
    flat[:3, 3] = 0.0                # every direction in the image plane: rank 2
    cases.append(("rank-2 inv_proj", w, h, c2w, flat, False))
    cases.append(("fov 179.9", w, h, *Camera(fov=179.9).uniforms(w, h), False))
    return cases


# ------------------------------------------------------------------ the driver
def _write(path, lists, cams):
    out = [np.array([bm.HOST_MAGIC, len(lists) + len(cams)], np.uint32)]
    for _, lo, first, depth, back, budget, _ in lists:
        out.append(np.array([0, len(lo), depth, back, budget], np.int64).astype(np.uint32))
        out += [np.asarray(lo, np.uint32), np.asarray(first, np.uint32)]
    for _, w, h, c2w, ip, _ in cams:
        out += [np.array([1, w, h], np.uint32), _cam_words(c2w, ip)]
    np.concatenate(out).astype("<u4").tofile(path)


def _read(path, n_lists, n_cams):
    w = np.fromfile(path, "<u4")
    assert w[0] == bm.HOST_MAGIC and w[1] == n_lists + n_cams
    at, lists, cams = 2, [], []
    for _ in range(n_lists):
        assert w[at] == 0
        listed, fine, cnt = (int(v) for v in w[at + 1:at + 4])
        lists.append((listed, fine, w[at + 4:at + 4 + 2 * cnt].reshape(-1, 2)))
        at += 4 + 2 * cnt
    for _ in range(n_cams):
        assert w[at] == 1
        f = w[at + 2:at + 26].view(np.float32)
        cams.append((int(w[at + 1]), f[:3], f[3:12].reshape(3, 3), f[12:24].reshape(4, 3)))
        at += 26
    assert at == len(w)
    return lists, cams


@pytest.fixture(scope="module")
def runs(tmp_path_factory, text_svo):
    if GXX is None or not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("g++ with the HIP headers not available")
    d = tmp_path_factory.mktemp("beam_host")
    lists, cams = list_cases(text_svo), camera_cases()
    _write(d / "cases.bin", lists, cams)
    out = {}
    for name, flags in (("plain", []), ("asan_ubsan", SAN)):
        exe = str(d / f"beam_host_{name}")
        cmd = [GXX, "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-D__HIP_PLATFORM_AMD__", "-isystem", HIP_INC,
               "-I", os.path.join(ROOT, "raytracingtest_amd", "csrc"), os.path.join(ROOT, "tests", "beam_host_driver.cpp"),
               "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            out[name] = (None, r.stderr)
            continue
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        res = str(d / f"results_{name}.bin")
        r = subprocess.run([exe, str(d / "cases.bin"), res], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
            (name, r.stdout[-400:], r.stderr[-3000:])
        out[name] = (_read(res, len(lists), len(cams)), "")
    assert out["plain"][0] is not None, out["plain"][1][-3000:]
    return lists, cams, out


def test_sanitized_run_agrees(runs):
    """The driver under ASan + UBSan ends clean (checked when it ran) and gives the same words."""
    _, _, out = runs
    if out["asan_ubsan"][0] is None:
        pytest.skip(f"sanitizer toolchain unavailable: {out['asan_ubsan'][1][-400:]}")
    (pl, pc), (sl, sc) = out["plain"][0], out["asan_ubsan"][0]
    assert len(pl) == len(sl) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(pl, sl))
    assert all(a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])) for a, b in zip(pc, sc))


def test_splat_lists_equal_the_model(runs):
    lists, _, out = runs
    got, _ = out["plain"][0]
    assert len(lists) > 50
    findings = []
    for (name, lo, first, depth, back, budget, leaves), (listed, fine, words) in zip(lists, got):
        want = bm.splat_list_model(lo, first, depth, back, budget)
        if want is None:
            if listed or len(words) or fine:
                findings.append(f"{name}: a list where the model has none")
            continue
        rows = bm.box_rows(words)
        if not listed or len(rows) != len(want):
            findings.append(f"{name}: {len(rows)} boxes, model {len(want)}")
            continue
        key = lambda r: [bm.morton16(*b) for b in r.tolist()]
        kg, kw = key(rows), key(want)
        if kg != kw or kg != sorted(kg):
            findings.append(f"{name}: Morton keys differ or are out of order")
        # equal keys: any order -- compare as sorted (key, box) rows
        if sorted(zip(kg, map(tuple, rows.tolist()))) != sorted(zip(kw, map(tuple, want.tolist()))):
            findings.append(f"{name}: boxes differ")
        if fine != (int(rows[:, 3].max()) if len(rows) else 0):
            findings.append(f"{name}: finest_box_depth {fine}")
        findings += [f"{name}: {f}" for f in bm.list_findings(rows, leaves, min(depth - back, 16))]
    assert not findings, findings[:20]


def test_list_cases_reach_their_rules(text_svo):
    """The model alone: nulls at back >= depth, leaves above ds listed at their own depth, the cut pool drops
    boxes, the budget coarsens the DAG's list and the DAG expands its shared subtree at two positions."""
    pools = _pools(text_svo)
    for name, (lo, first, depth, _) in pools.items():
        assert bm.splat_list_model(lo, first, depth, depth) is None and bm.splat_list_model(lo, first, depth, depth + 3) is None
        one = bm.splat_list_model(lo, first, depth, depth - 1)
        assert one is not None and set(one[:, 3].tolist()) == {1}, name
    lo, first, depth, _ = pools["mixed"]
    assert len(set(bm.splat_list_model(lo, first, depth, 1)[:, 3].tolist())) >= 3      # leaves at several depths above ds
    lo, first, depth, _ = pools["dag"]
    assert depth == 9
    full, small = bm.splat_list_model(lo, first, depth, 0), bm.splat_list_model(lo, first, depth, 0, 64)
    assert len(small) < len(full) and small[:, 3].max() < full[:, 3].max() and len(small) >= 64
    assert len(full) > 2 * (len(lo) - 4) // 8                 # more boxes than one copy of S could give
    lo5, first5, depth5, _ = pools["random5"]
    cut = pools["cut"]
    assert len(bm.splat_list_model(cut[0], cut[1], depth5, 0)) < len(bm.splat_list_model(lo5, first5, depth5, 0))
    assert pools["text"][2] > 2 and pools["random9"][2] == 9


def test_list_findings_reject_wrong_lists():
    leaves = np.array([[0, 0, 0, 2], [3, 3, 3, 2], [1, 0, 0, 1]])
    good = np.array([[0, 0, 0, 1], [1, 1, 1, 1], [1, 0, 0, 1]])
    assert bm.list_findings(good, leaves, 1) == []
    assert bm.list_findings(good[:2], leaves, 1)                                   # a leaf in no box
    assert bm.list_findings(np.vstack([good, [[0, 0, 0, 2]]]), leaves, 2)          # a box inside another
    assert bm.list_findings(np.vstack([good, good[:1]]), leaves, 1)                # a box twice
    assert bm.list_findings(np.array([[0, 0, 0, 2], [3, 3, 3, 2], [1, 0, 0, 1]]), leaves, 1)   # deeper than ds


def test_beam_camera_equals_the_model(runs):
    _, cams, out = runs
    _, got = out["plain"][0]
    ran = 0
    for (name, w, h, c2w, ip, accept), (ok, org, minv, plane) in zip(cams, got):
        cm = bm.beam_camera_model(c2w, ip, w, h)
        assert (cm is not None) == accept, f"{name}: the model's own refusal"
        assert bool(ok) == accept, f"{name}: accepted = {ok}"
        if not accept:
            continue
        ran += 1
        M = cm["M"]
        prod = M @ minv.astype(np.float64)
        scale = np.abs(M).sum(1)[:, None] * np.abs(minv.astype(np.float64)).sum(0)[None, :]   # the row's terms
        assert np.all(np.abs(prod - np.eye(3)) <= 1e-5 * np.maximum(scale, 1.0)), f"{name}: M minv = {prod}"
        assert org.tobytes() == cm["org"].tobytes(), f"{name}: org {org} != {cm['org']}"
        D = cm["corners"] / np.linalg.norm(cm["corners"], axis=1, keepdims=True)
        mid = cm["mid"] / np.linalg.norm(cm["mid"])
        for j in range(4):
            n = plane[j].astype(np.float64)
            assert abs(np.linalg.norm(n) - 1.0) < 1e-6, name
            assert abs(n @ D[j]) < 1e-6 and abs(n @ D[(j + 1) % 4]) < 1e-6, f"{name}: plane {j} misses its corners"
            assert n @ mid > 0.0, f"{name}: plane {j} faces outwards"
        assert np.allclose(plane, cm["plane"], rtol=0, atol=1e-6), name
    assert ran == 18


def test_header_has_no_hip_call():
    """Host code only: svo_traverse.h (for Camera and BeamParams) is the one project header, and no hip*( call."""
    import re
    with open(os.path.join(ROOT, "raytracingtest_amd", "csrc", "svo_beam.h")) as f:
        src = f.read()
    assert [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include \"")] == ['"svo_traverse.h"']
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
