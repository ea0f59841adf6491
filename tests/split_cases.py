"""Shared geometry of the split tests (tests/test_split_cases.py on the CPU, tests/test_gpu_split.py on the
GPU): frames that are no multiple of the 8x8 tile, band heights that are no multiple of it either, deals
that leave a rank without rows -- and the host statements the GPU's bytes are compared with.  No GPU is
needed to import this module; the buffer maker takes torch as an argument.

Pool: build_menger(7).  Pose "edge": the overview eye looking at (-6, -6, 0) through a 30 degree lens, so
that the frame's last tile column and last tile row -- the partial ones -- hold hits, misses, lit and
shadowed pixels (the overview pose itself leaves them all sky; tests/test_split_cases.py asserts the counts
on the oracle).

Frames: A = 203 x 77 (26 tile columns: the raster path; a 3-pixel partial column, a 5-row partial row;
width % 4 == 3: the per-pixel assemble kernel), B = 124 x 45 (16 tile columns: XCD strips and the segmented
kernel; 4 and 5; width % 4 == 0: the uint4 assemble kernel).

Deals: band heights 1, 3, 5 (a tile's 8 local rows come from several bands), 8 (the control), 12 (a band
starts in the middle of a tile), 50 (ranks without rows); 2 and 3 ranks round-robin and 3 ranks dealt by the
owner cycle (0, 1, 1, 2, 1), whose length is no power of two."""
import numpy as np

from raytracingtest_amd import band_rows
from raytracingtest_amd.camera import OVERVIEW_EYE, main_light, overview_camera

POOL_NAME = "menger7"          # the cache name of the pool in tests/reflect_util.py and tests/ambient_util.py
POOL_DEPTH = 7
POOL_NODES = 149601
EDGE_TARGET = (-6.0, -6.0, 0.0)
EDGE_FOV = 30.0
FRAMES = {"A": (203, 77), "B": (124, 45)}
HEIGHTS = (1, 3, 5, 8, 12, 50)
WEIGHTED = (0, 1, 1, 2, 1)
SPLITS = {"rr2": (2, None), "rr3": (3, None), "w3": (3, WEIGHTED)}
DEALS = tuple((rows, split) for rows in HEIGHTS for split in SPLITS)
GUARD_BYTES = 4096
FILL = 0xA5
# bytes per pixel of the per-pixel outputs of svo_frame; hitmask is one uint64 per band-local tile
ITEM = {"hits": 24, "rgba": 16, "rgba8": 4, "compact": 12, "position": 16, "voxel": 8, "rgb8": 3}
FRAME_KEYS = tuple(ITEM) + ("hitmask",)
COLOUR_KEYS = ("rgba", "rgba8", "rgb8")

_cache = {}


def edge_camera():
    cam = overview_camera(OVERVIEW_EYE, target=EDGE_TARGET)
    cam.fov = EDGE_FOV
    return cam


def pool():
    if "pool" not in _cache:
        from raytracingtest_amd.builder import build_menger
        _cache["pool"] = build_menger(POOL_DEPTH)
    return _cache["pool"]


# ------------------------------------------------------------------------------------------ deals
def band_of(rows, rank, split):
    """The svo_band tuple of `rank` under band height `rows` and the split `split` (a key of SPLITS)."""
    count, owner = SPLITS[split]
    return (rows, rank, count) if owner is None else (rows, rank, count, owner)


def ranks(split):
    return range(SPLITS[split][0])


def rows_of(height, band):
    """The frame rows of a deal's rank, in order (None: the whole frame)."""
    return np.arange(height) if band is None else band_rows(height, band)


def n_tiles(width, n_rows):
    return ((width + 7) // 8) * ((n_rows + 7) // 8)


def empty_triples():
    """Every (frame, (rows, split), rank) whose rank owns no row."""
    return [(f, (rows, split), r) for f, (_, h) in FRAMES.items() for rows, split in DEALS for r in ranks(split)
            if len(rows_of(h, band_of(rows, r, split))) == 0]


# ------------------------------------------------------------------------------------------ the oracle's frames
def oracle_frame(oracle_mod, frame, mode=0, shadows=False, svo=None, camera=None, name=POOL_NAME):
    """The oracle's whole frame (computed once per case, read-only) as a dict of [height, width, ...] arrays:
    the seven per-pixel outputs of svo_frame and `hit`, the hit flags.  svo / camera / name: another pool and
    pose than the module's (name keys the cache)."""
    key = ("frame", name, frame, int(mode), bool(shadows))
    if key not in _cache:
        w, h = FRAMES[frame]
        svo = pool() if svo is None else svo
        c2w, inv_proj = (edge_camera() if camera is None else camera).uniforms(w, h)
        ocam = oracle_mod.make_camera(c2w, inv_proj, (0.5, 0.5), main_light())
        osvo = oracle_mod.OracleSVO(nodes=svo.to_v2(), attachments=svo.attachments)
        hits, rgba, _, pos, vox = oracle_mod.render_ex(osvo, ocam, w, h, mode | (oracle_mod.SHADOW_RAYS if shadows else 0))
        _cache[key] = frame_outputs(oracle_mod, hits, rgba, pos, vox, w, h)
    return _cache[key]


def frame_outputs(oracle_mod, hits, rgba, pos, vox, w, h):
    """Records, Result, position and voxel keys of a frame -> every per-pixel output, [h, w, ...], read-only."""
    rgba = np.ascontiguousarray(rgba, np.float32).reshape(h * w, 4)
    words = oracle_mod.pack_rgba8(rgba)
    out = {"hits": hits.reshape(h, w), "rgba": rgba.reshape(h, w, 4), "rgba8": words.reshape(h, w),
           "compact": np.ascontiguousarray(hits.view(np.uint8).reshape(h, w, 24)[:, :, :12]),
           "rgb8": np.ascontiguousarray(words.view(np.uint8).reshape(h, w, 4)[:, :, :3]),
           "hit": ((hits["flags"] & 1) != 0).reshape(h, w)}
    if pos is not None:
        out["position"] = pos.reshape(h, w, 4)
    if vox is not None:
        out["voxel"] = vox.reshape(h, w)
    for v in out.values():
        v.setflags(write=False)
    return out


def with_colours(oracle_mod, ref, rgba):
    """`ref` (an oracle_frame) with the colour outputs of another Result (a model's expected frame)."""
    h, w = ref["hit"].shape
    rgba = np.ascontiguousarray(rgba, np.float32).reshape(h * w, 4)
    words = oracle_mod.pack_rgba8(rgba)
    out = dict(ref)
    out.update(rgba=rgba.reshape(h, w, 4), rgba8=words.reshape(h, w),
               rgb8=np.ascontiguousarray(words.view(np.uint8).reshape(h, w, 4)[:, :, :3]))
    return out


def expected_rows(ref, ys, key):
    """The bytes a band render of the rows `ys` must leave in output `key` (band layout)."""
    if key == "hitmask":
        return expected_masks(ref["hit"][ys], ref["hit"].shape[1]).tobytes()
    return np.ascontiguousarray(ref[key][ys]).tobytes()


# ------------------------------------------------------------------------------------------ band-local tiles
def expected_masks(hit_rows, width):
    """svo_frame.hitmask of a band: hit_rows [R, width] are the hit flags of the band's rows in order; tile
    (lr // 8, x // 8) of the band's LOCAL rows lr, row-major with ceil(width / 8) tiles per tile row, has bit
    (lr % 8) * 8 + x % 8 set for a hit.  R = 0: no word."""
    hit_rows = np.asarray(hit_rows, bool).reshape(-1, width)
    tx = (width + 7) // 8
    masks = np.zeros(n_tiles(width, len(hit_rows)), np.uint64)
    lr, x = np.nonzero(hit_rows)
    bit = ((lr & 7) * 8 + (x & 7)).astype(np.uint64)
    np.bitwise_or.at(masks, (lr >> 3) * tx + (x >> 3), np.uint64(1) << bit)
    return masks


def expected_sparse_part(hit_rows, rgb_rows, width):
    """The sparse payload of a band (svo_rt.h, svo_pack_hits): `masks` (expected_masks), `offsets` (uint32, the
    hits before each tile, then the band's count: n_tiles + 1 entries), `count`, `rgb` [count, 3] (the hit
    pixels' RGB tile by tile, lanes in row-major order) and `bytes`, the part as it is sent."""
    hit_rows = np.asarray(hit_rows, bool).reshape(-1, width)
    rgb_rows = np.asarray(rgb_rows, np.uint8).reshape(len(hit_rows), width, 3)
    tx = (width + 7) // 8
    n = n_tiles(width, len(hit_rows))
    masks = expected_masks(hit_rows, width)
    lr, x = np.nonzero(hit_rows)
    tile, lane = (lr >> 3) * tx + (x >> 3), (lr & 7) * 8 + (x & 7)
    per_tile = np.bincount(tile, minlength=n)[:n] if n else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], np.cumsum(per_tile)]).astype(np.uint32)
    order = np.lexsort((lane, tile))
    rgb = np.ascontiguousarray(rgb_rows[lr[order], x[order]]).reshape(-1, 3)
    return {"masks": masks, "offsets": offsets, "count": int(offsets[-1]), "rgb": rgb,
            "bytes": masks.tobytes() + offsets.tobytes() + rgb.tobytes()}


# ------------------------------------------------------------------------------------------ guarded buffers
class Arena:
    """Named device buffers in one allocation, each followed by a guard of at least GUARD_BYTES; buffers and
    guards alike start out filled with FILL, a byte pattern no render leaves in a whole pixel.  A buffer of 0
    bytes is its guard alone: a valid pointer whose every byte must stay FILL (an empty rank's part).

    reset() refills, ptr(name) is the device pointer, fetch() copies the allocation to the host (after the
    caller synchronised the context), get(name) is a buffer's bytes in that copy and check_guards() asserts
    that every byte outside the buffers still holds FILL: a small overrun fails here instead of faulting."""

    def __init__(self, torch, sizes, device="cuda"):
        self.torch = torch
        self.device = device
        self.span = {}
        pos = 0
        for name, nbytes in sizes.items():
            self.span[name] = (pos, int(nbytes))
            pos = (pos + int(nbytes) + GUARD_BYTES + 255) & ~255
        self.t = torch.empty(max(pos, GUARD_BYTES), dtype=torch.uint8, device=device)
        self.inside = np.zeros(self.t.numel(), bool)
        for o, n in self.span.values():
            self.inside[o:o + n] = True
        self.host = None
        self.reset()

    def sync(self):
        if self.device != "cpu":   # "cpu": the helper's own test
            self.torch.cuda.synchronize()

    def reset(self):
        self.t.fill_(FILL)
        self.sync()   # the fill runs on torch's stream, the renders on the context's
        self.host = None

    def zero(self, name):
        o, n = self.span[name]
        self.t[o:o + n].zero_()
        self.sync()

    def ptr(self, name):
        return self.t.data_ptr() + self.span[name][0]

    def ptrs(self, names=None):
        return {k: self.ptr(k) for k in (self.span if names is None else names)}

    def fetch(self):
        self.sync()
        self.host = self.t.cpu().numpy().copy()
        return self

    def get(self, name):
        o, n = self.span[name]
        return self.host[o:o + n]

    def check_guards(self, what=""):
        bad = np.flatnonzero(~self.inside & (self.host != FILL))
        if len(bad):
            first = int(bad[0])
            owner = max((o + n, k) for k, (o, n) in self.span.items() if o + n <= first)[1]
            raise AssertionError(f"{what}: {len(bad)} guard bytes written, the first {first - sum(self.span[owner])} "
                                 f"bytes behind the end of {owner!r}")

    def untouched(self, name):
        return bool(np.all(self.get(name) == FILL))


def band_sizes(width, height, band, keys, layout_frame=False):
    """Buffer sizes of a band render's outputs: band layout holds the rank's rows, frame layout the frame; the
    hit mask is band-local in both."""
    rows = len(rows_of(height, band))
    px = (height if layout_frame else rows) * width
    return {k: n_tiles(width, rows) * 8 if k == "hitmask" else px * ITEM[k] for k in keys}
