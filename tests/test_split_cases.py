"""The inputs of tests/test_gpu_split.py, qualified on the CPU oracle (mode 0, shadow rays on), and the
host helpers of tests/split_cases.py checked against the two statements the suite already had: tile_masks
(tests/test_gpu_lod.py) and the sparse part of tests/test_distributed.py.

Every condition is asserted on the reference, never on a kernel's output: a GPU test that compares a band
with the oracle proves something only where that band holds hits and misses, lit and shadowed pixels -- and
the partial edge tiles prove something only if they are not all sky, which is what the overview pose gives."""
import numpy as np
import pytest

from tests import split_cases as sc


@pytest.fixture(scope="module")
def frames(oracle_mod):
    return {f: sc.oracle_frame(oracle_mod, f, 0, shadows=True) for f in sc.FRAMES}


def _classes(ref, sel):
    """(hits, misses, shadowed hits, lit hits) among the pixels `sel` selects."""
    hit = ref["hit"][sel]
    shadow = (ref["hits"]["flags"][sel] & 8) != 0
    return int(hit.sum()), int((~hit).sum()), int((hit & shadow).sum()), int((hit & ~shadow).sum())


def test_pool_and_pose():
    from raytracingtest_amd.camera import OVERVIEW_EYE
    from tests import ambient_util, reflect_util
    assert len(sc.pool()) == sc.POOL_NODES
    cam = reflect_util.POSES["edge"]()
    assert cam.fov == 30.0 and tuple(cam.position) == OVERVIEW_EYE
    fwd = np.asarray(sc.EDGE_TARGET) - np.asarray(OVERVIEW_EYE)
    assert np.allclose(cam.rotation[:, 2], fwd / np.linalg.norm(fwd))
    assert ambient_util.ru.POSES is reflect_util.POSES   # ambient_util reaches the pose through reflect_util


def test_frames_take_the_intended_paths():
    (wa, ha), (wb, hb) = sc.FRAMES["A"], sc.FRAMES["B"]
    assert (wa + 7) // 8 == 26 and wa % 8 == 3 and ha % 8 == 5 and wa % 4 == 3
    assert (wb + 7) // 8 == 16 and wb % 8 == 4 and hb % 8 == 5 and wb % 4 == 0
    assert len(sc.WEIGHTED) & (len(sc.WEIGHTED) - 1) != 0 and set(sc.WEIGHTED) == {0, 1, 2}
    assert 8 in sc.HEIGHTS and len(sc.DEALS) == 18


def test_hit_share(frames):
    for f, ref in frames.items():
        share = float(ref["hit"].mean())
        print(f, "hit share", round(share, 3))
        assert 0.5 <= share <= 0.9


def test_partial_tiles_hold_every_class(frames):
    """The partial tile column and the partial tile row of each frame: hits, misses, shadowed and lit hits."""
    for f, ref in frames.items():
        w, h = sc.FRAMES[f]
        col = np.zeros((h, w), bool)
        col[:, w - w % 8:] = True
        row = np.zeros((h, w), bool)
        row[h - h % 8:, :] = True
        for name, sel in (("column", col), ("row", row)):
            hits, misses, shadowed, lit = _classes(ref, sel)
            print(f, name, hits, misses, shadowed, lit)
            assert hits >= 40 and misses >= 40 and shadowed >= 40 and lit >= 30


def test_every_rank_with_rows_holds_every_class(frames):
    low = 1 << 30
    for f, ref in frames.items():
        h = sc.FRAMES[f][1]
        for rows, split in sc.DEALS:
            for r in sc.ranks(split):
                ys = sc.rows_of(h, sc.band_of(rows, r, split))
                if len(ys) == 0:
                    continue
                counts = _classes(ref, ys)
                low = min(low, *counts)
                assert min(counts) >= 100, (f, rows, split, r, counts)
    print("the smallest class of a rank:", low)


def test_deals_cover_the_frame_and_leave_the_empty_ranks():
    for f, (_, h) in sc.FRAMES.items():
        for rows, split in sc.DEALS:
            seen = np.concatenate([sc.rows_of(h, sc.band_of(rows, r, split)) for r in sc.ranks(split)])
            assert np.array_equal(np.sort(seen), np.arange(h))
    empty = sc.empty_triples()
    assert len(empty) == 7 and all(rows == 50 for _, (rows, _), _ in empty)
    assert sorted(t for t in empty if t[0] == "A") == [("A", (50, "rr3"), 2), ("A", (50, "w3"), 2)]
    assert sorted(t for t in empty if t[0] == "B") == [("B", (50, "rr2"), 1), ("B", (50, "rr3"), 1), ("B", (50, "rr3"), 2),
                                                       ("B", (50, "w3"), 1), ("B", (50, "w3"), 2)]


def test_models_change_pixels_in_both_edge_strips(oracle_mod, frames):
    """The reflection and ambient models run with the pose at both frames and change pixels in the partial
    tile column and in the partial tile row, so a pass that skipped (or overran) them would show."""
    from tests import ambient_util as au
    from tests import reflect_util as ru
    svo = sc.pool()
    for f, (w, h) in sc.FRAMES.items():
        base = ru.primary(oracle_mod, sc.POOL_NAME, svo, "edge", w, h)["rgba"].reshape(h, w, 4)
        assert base.tobytes() == sc.oracle_frame(oracle_mod, f, 0)["rgba"].tobytes()
        refl = ru.expected_frame(oracle_mod, sc.POOL_NAME, svo, "edge", w, h).reshape(h, w, 4)
        amb = au.expected_frame(oracle_mod, sc.POOL_NAME, svo, "edge", w, h, n_rays=4, variant=3).reshape(h, w, 4)
        for name, model in (("reflection", refl), ("ambient", amb)):
            changed = (model != base).any(axis=2)
            col, row = int(changed[:, w - w % 8:].sum()), int(changed[h - h % 8:, :].sum())
            print(f, name, "changed pixels in the column / row strip:", col, row)
            assert col >= 100 and row >= 300


# ------------------------------------------------------------------------------------------ the helpers
def test_masks_and_sparse_part_agree_with_the_existing_statements(frames):
    """On whole frames (band-local tiles = frame tiles) expected_masks is tile_masks and expected_sparse_part
    is test_distributed's host restatement; on a deal's rows the masks are tile_masks of the gathered rows."""
    from tests.test_distributed import _sparse_part
    from tests.test_gpu_lod import tile_masks
    for f, ref in frames.items():
        w, h = sc.FRAMES[f]
        hit, rgb = ref["hit"], ref["rgb8"]
        assert np.array_equal(sc.expected_masks(hit, w), tile_masks(hit, w, h))
        part = sc.expected_sparse_part(hit, rgb, w)
        assert part["bytes"] == _sparse_part(hit, rgb)
        assert part["count"] == int(hit.sum()) == len(part["rgb"])
        assert len(part["offsets"]) == sc.n_tiles(w, h) + 1 and len(part["bytes"]) == 12 * sc.n_tiles(w, h) + 4 + 3 * part["count"]
        for rows, split in ((3, "w3"), (12, "rr2"), (50, "rr3")):
            for r in sc.ranks(split):
                ys = sc.rows_of(h, sc.band_of(rows, r, split))
                assert np.array_equal(sc.expected_masks(hit[ys], w), tile_masks(hit[ys], w, len(ys)))
                if len(ys):
                    assert sc.expected_sparse_part(hit[ys], rgb[ys], w)["bytes"] == _sparse_part(hit[ys], rgb[ys])


def test_masks_by_hand():
    """Width 10 (two tile columns), 9 rows (two tile rows): single pixels land on the bits the header names."""
    hit = np.zeros((9, 10), bool)
    hit[0, 0] = hit[7, 7] = hit[3, 9] = hit[8, 1] = hit[8, 8] = True
    m = sc.expected_masks(hit, 10)
    assert m.tolist() == [1 | 1 << 63, 1 << (3 * 8 + 1), 1 << 1, 1 << 0]
    rgb = np.arange(9 * 10 * 3, dtype=np.uint8).reshape(9, 10, 3)
    part = sc.expected_sparse_part(hit, rgb, 10)
    assert part["offsets"].tolist() == [0, 2, 3, 4, 5]
    assert part["rgb"].tolist() == [rgb[0, 0].tolist(), rgb[7, 7].tolist(), rgb[3, 9].tolist(), rgb[8, 1].tolist(),
                                    rgb[8, 8].tolist()]
    empty = sc.expected_sparse_part(np.zeros((0, 10), bool), np.zeros((0, 10, 3), np.uint8), 10)
    assert empty["bytes"] == b"\0\0\0\0" and len(sc.expected_masks(np.zeros((0, 10), bool), 10)) == 0


def test_arena_guards_catch_an_overrun():
    """The guarded buffer maker on host memory: at least 4 KiB of pattern behind every buffer, an empty
    buffer is a valid pointer to its guard, a byte written behind a buffer fails check_guards and names the
    buffer, a byte written inside one does not."""
    torch = pytest.importorskip("torch")
    arena = sc.Arena(torch, {"a": 1000, "empty": 0, "b": 24}, device="cpu")
    spans = sorted(arena.span.values())
    for (o, n), (o2, _) in zip(spans, spans[1:] + [(arena.t.numel(), 0)]):
        assert o2 - (o + n) >= sc.GUARD_BYTES and o % 256 == 0
    assert arena.ptr("empty") == arena.t.data_ptr() + arena.span["empty"][0] and arena.ptr("empty") != arena.ptr("b")
    arena.fetch().check_guards("fresh")
    assert arena.untouched("a") and len(arena.get("empty")) == 0
    arena.t[arena.span["a"][0] + 999] = 0
    arena.zero("b")
    arena.fetch().check_guards("written inside")
    assert not arena.untouched("a") and not arena.get("b").any()
    arena.t[arena.span["a"][0] + 1000 + 3] = 7          # 4 bytes behind the end of "a"
    with pytest.raises(AssertionError, match=r"1 guard bytes written, the first 3 bytes behind the end of 'a'"):
        arena.fetch().check_guards("overrun")
    arena.reset()
    arena.t[arena.span["empty"][0]] = 0                 # an empty part's first byte
    with pytest.raises(AssertionError, match=r"behind the end of 'empty'"):
        arena.fetch().check_guards("empty part written")
    arena.reset()
    arena.t[arena.t.numel() - 1] = 1                    # the last guard byte of the last buffer
    with pytest.raises(AssertionError, match=r"behind the end of 'b'"):
        arena.fetch().check_guards("far overrun")


def test_band_sizes():
    w, h = sc.FRAMES["A"]
    band = sc.band_of(5, 1, "w3")
    n = len(sc.rows_of(h, band))
    assert n == 45   # bands 1, 2, 4 of each cycle of 5, three cycles; the 2-row band 15 is rank 0's
    s = sc.band_sizes(w, h, band, sc.FRAME_KEYS)
    assert s["hits"] == n * w * 24 and s["hitmask"] == 26 * ((n + 7) // 8) * 8
    assert sc.band_sizes(w, h, band, ("rgba8",), layout_frame=True)["rgba8"] == w * h * 4
    assert set(sc.band_sizes(*sc.FRAMES["B"], sc.band_of(50, 1, "rr2"), sc.FRAME_KEYS).values()) == {0}
