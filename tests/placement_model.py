"""Plain numpy models of the placement-only kernels (csrc/svo_kernel.hip: order_tiles_kernel,
order_strips_kernel, query_keys_kernel + the radix sort), written from the rules the headers state
(csrc/svo_traverse.h), and the checks that compare a kernel's output buffers with them.

TEST INFRASTRUCTURE ONLY.  Whatever these kernels write, a frame or a ray batch comes out the same;
only its time changes.  So their outputs are compared here, word by word, with a model.  Everything
is integer-exact; the checks return a list of findings (empty: the buffers are right).

The checks leave exactly this much free, because the kernels do:
  * tile order: the order of the tiles inside one class;
  * strip order: the order of the tiles inside one class of one XCD, and WHICH tiles of a class are
    the segmented ones (an LDS atomic decides) -- not how many, not where, not their codes;
  * query sort: the order of equal keys.

The case file of tests/placement_driver.cpp is written and its result file read here too.
"""
import numpy as np

from tests.lod_tracer import ray_setup

GUARD = 0xA5C3F00D
GUARD_WORDS = 64
SEG_COST_FLAG = 0x8000
SEG_EMPTY = 0xFFFFFFFF
SEG_KMAX = 8
ORDER_CHUNK = 1024 * 32
QUERY_RAW = 2
KEY_NONE = (1 << 30) - 1
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1
MAGIC = 0x31434C50


# ------------------------------------------------------------------ sizes (svo_traverse.h)
def seg_kmax_of(kpack):
    return max([1] + [(kpack >> (4 * c)) & 15 for c in range(6)])


def order_strips_grid(n, seg_cap, kmax):
    return n + 8 * (kmax - 1) * seg_cap


def order_strips_entries(n, seg_cap, kmax):
    return order_strips_grid(n, seg_cap, kmax) + 36


def order_cost_capacity(n):
    return (n + ORDER_CHUNK - 1) // ORDER_CHUNK * ORDER_CHUNK


def _guard_findings(buf, words, what):
    buf = np.asarray(buf, np.uint32)
    if len(buf) != words + GUARD_WORDS:
        return [f"{what}: {len(buf)} words, not {words} + {GUARD_WORDS}"]
    bad = np.flatnonzero(buf[words:] != GUARD)
    return [f"{what}: guard word {int(bad[0])} overwritten with {int(buf[words + bad[0]]):#x}"] if len(bad) else []


def untouched(buf):
    """A buffer no kernel wrote: every word still the fill pattern."""
    return bool(np.all(np.asarray(buf, np.uint32) == GUARD))


# ------------------------------------------------------------------ tile order
def tile_order_model(cost, n):
    """cost: the u16 cost words (at least n).  Classes of the n tiles against mx = max cost:
    0 if 2k >= mx, 1 if 4k >= mx, 2 if 8k >= mx, else 3."""
    k = (np.asarray(cost, np.uint16)[:n].astype(np.int64)) & 0x7FFF
    mx = int(k.max())
    cls = np.full(n, 3, np.int64)
    cls[8 * k >= mx] = 2
    cls[4 * k >= mx] = 1
    cls[2 * k >= mx] = 0
    tiles = [np.flatnonzero(cls == q) for q in range(4)]
    ends = np.cumsum([len(t) for t in tiles])
    stats = np.zeros(16, np.uint32)
    stats[0] = mx
    stats[1] = int(k.sum()) & 0xFFFFFFFF
    return {"n": n, "tiles": tiles, "ends": ends.astype(np.uint32), "stats": stats, "cls": cls}


def check_tile_order(order, stats, model, with_stats=True):
    n = model["n"]
    out = _guard_findings(order, n + 4, "order") + _guard_findings(stats, 16, "stats")
    if out:
        return out
    order, stats = np.asarray(order, np.uint32), np.asarray(stats, np.uint32)
    if not np.array_equal(order[n:n + 4], model["ends"]):
        out.append(f"class ends {order[n:n + 4].tolist()}, expected {model['ends'].tolist()}")
    lo = 0
    for q in range(4):
        hi = int(model["ends"][q])
        if not np.array_equal(np.sort(order[lo:hi]), model["tiles"][q]):
            out.append(f"class {q}: entries [{lo}, {hi}) are not the class's tiles")
        lo = hi
    if with_stats:
        if not np.array_equal(stats[:16], model["stats"]):
            out.append(f"stats {stats[:16].tolist()}, expected {model['stats'].tolist()}")
    elif not untouched(stats):
        out.append("stats written although null was passed")
    return out


# ------------------------------------------------------------------ strip order
def strip_refusal(n, tiles_x, seg_cap, kpack):
    """launch_order_strips returns hipErrorInvalidValue without a launch for these."""
    if any(((kpack >> (4 * c)) & 15) not in (0, 4, 8) for c in range(6)):
        return True
    if seg_cap > 0 and n % tiles_x != 0:
        return True
    return seg_cap > 0 and order_strips_grid(n, seg_cap, seg_kmax_of(kpack)) >= (1 << 28)


def tile_costs(cost, n, part_cost=None):
    """The cost of every tile: word & 0x7FFF, or for a flagged word (with part_cost given) the max
    of the tile's first 4 part costs, of all 8 when word & 15 == 8."""
    w = np.asarray(cost, np.uint16)[:n].astype(np.int64)
    k = w & 0x7FFF
    if part_cost is not None:
        pc = np.asarray(part_cost, np.uint16)[:SEG_KMAX * n].reshape(n, SEG_KMAX).astype(np.int64)
        seg = np.where((w & 15) == 8, pc.max(axis=1), pc[:, :4].max(axis=1))
        k = np.where((w & SEG_COST_FLAG) != 0, seg, k)
    return k


def strip_order_model(cost, n, tiles_x, seg_cap=0, kpack=0, spread=0, part_cost=None):
    assert n % 8 == 0 and n % tiles_x == 0 and tiles_x % 8 == 0 and not strip_refusal(n, tiles_x, seg_cap, kpack)
    tiles_y = n // tiles_x
    kmax = seg_kmax_of(kpack)
    L = n // 8 + (kmax - 1) * seg_cap
    k = tile_costs(cost, n, part_cost).reshape(tiles_y, tiles_x)
    cc = k
    if spread:   # the heaviest of the 3x3 neighbourhood, clipped at the frame's edges
        pad = np.zeros((tiles_y + 2, tiles_x + 2), np.int64)
        pad[1:-1, 1:-1] = k
        cc = np.max([pad[1 + dy:1 + dy + tiles_y, 1 + dx:1 + dx + tiles_x] for dy in (-1, 0, 1) for dx in (-1, 0, 1)],
                    axis=0)
    tile_id = np.arange(n, dtype=np.int64).reshape(tiles_y, tiles_x)
    K = [(kpack >> (4 * c)) & 15 for c in range(6)]
    stats = np.zeros(16, np.uint32)
    xcds = []
    for x in range(8):
        own_k, own_c, own_t = k[:, x::8].reshape(-1), cc[:, x::8].reshape(-1), tile_id[:, x::8].reshape(-1)
        mx = int(own_k.max())
        stats[2 * x] = mx
        stats[2 * x + 1] = int(own_k.sum()) & 0xFFFFFFFF
        cls = np.full(len(own_c), 5, np.int64)
        cls[8 * own_c >= mx] = 4
        cls[4 * own_c >= mx] = 3
        cls[2 * own_c >= mx] = 2
        cls[4 * own_c >= 3 * mx] = 1
        cls[8 * own_c >= 7 * mx] = 0
        tiles = [np.sort(own_t[cls == c]) for c in range(6)]
        left, start, blocks = seg_cap, 0, []
        for c in range(6):
            cnt = len(tiles[c])
            segs = min(cnt, left) if K[c] > 1 else 0
            left -= segs
            end = start + cnt + (K[c] - 1) * segs if K[c] > 1 else start + cnt
            blocks.append({"start": start, "end": end, "segs": segs, "K": K[c], "tiles": tiles[c]})
            start = end
        xcds.append({"mx": mx, "blocks": blocks})
    return {"n": n, "L": L, "G": 8 * L, "kmax": kmax, "seg_cap": seg_cap, "xcds": xcds, "stats": stats}


def strip_order_layout(model, pick_last=False):
    """One buffer (without guard words) that satisfies the model: the segmented tiles of a class
    are its first (or last) ones.  For the CPU tests of check_strip_order."""
    G, L = model["G"], model["L"]
    o = np.full(G + 36, SEG_EMPTY, np.uint32)
    o[G:G + 4] = 0
    lst = o[:G].reshape(L, 8)
    for x, xc in enumerate(model["xcds"]):
        for c, b in enumerate(xc["blocks"]):
            t = b["tiles"][::-1] if pick_last else b["tiles"]
            seg, plain = t[:b["segs"]], t[b["segs"]:]
            j = b["start"]
            code0 = 1 if b["K"] == 4 else 5
            for tile in seg:
                lst[j:j + b["K"], x] = tile | ((code0 + np.arange(b["K"])) << 28)
                j += b["K"]
            lst[j:j + len(plain), x] = plain
            assert j + len(plain) == b["end"]
            if c >= 2:
                o[G + 4 + 4 * x + c - 2] = b["end"]
    return o


def check_strip_order(order, stats, model, with_stats=True):
    G, L = model["G"], model["L"]
    out = _guard_findings(order, G + 36, "order") + _guard_findings(stats, 16, "stats")
    if out:
        return out
    order, stats = np.asarray(order, np.uint32), np.asarray(stats, np.uint32)
    lst = order[:G].reshape(L, 8)
    if np.any(order[G:G + 4] != 0):
        out.append(f"global bounds {order[G:G + 4].tolist()}, expected zeros")
    for x, xc in enumerate(model["xcds"]):
        col = lst[:, x].astype(np.int64)
        ends = [b["end"] for b in xc["blocks"][2:]]
        got_ends = order[G + 4 + 4 * x:G + 8 + 4 * x].tolist()
        if got_ends != ends:
            out.append(f"XCD {x}: class ends {got_ends}, expected {ends}")
        for c, b in enumerate(xc["blocks"]):
            blk = col[b["start"]:b["end"]]
            ns = b["segs"] * b["K"]
            groups, plain = blk[:ns].reshape(b["segs"], b["K"]) if ns else np.zeros((0, 1), np.int64), blk[ns:]
            if ns:
                code0 = 1 if b["K"] == 4 else 5
                if not np.array_equal(groups >> 28, np.broadcast_to(code0 + np.arange(b["K"]), groups.shape)):
                    out.append(f"XCD {x} class {c}: part codes of the {b['segs']} groups at {b['start']} wrong")
                if np.any((groups & 0x0FFFFFFF) != (groups[:, :1] & 0x0FFFFFFF)):
                    out.append(f"XCD {x} class {c}: a group spans more than one tile")
            if np.any(plain >> 28):
                out.append(f"XCD {x} class {c}: a plain entry carries a part code (or is empty)")
            got = np.sort(np.concatenate([groups[:, 0] & 0x0FFFFFFF, plain])) if ns else np.sort(plain)
            if not np.array_equal(got, b["tiles"]):
                out.append(f"XCD {x} class {c}: block [{b['start']}, {b['end']}) does not hold the class's "
                           f"{len(b['tiles'])} tiles once each")
        tail = col[xc["blocks"][5]["end"]:]
        if np.any(tail != SEG_EMPTY):
            out.append(f"XCD {x}: entries behind the last class are not all SEG_EMPTY")
    if with_stats:
        if not np.array_equal(stats[:16], model["stats"]):
            out.append(f"stats {stats[:16].tolist()}, expected {model['stats'].tolist()}")
    elif not untouched(stats):
        out.append("stats written although null was passed")
    return out


# ------------------------------------------------------------------ query keys
def morton27(g):
    """Bit i of g[:, a] -> bit 3 i + a (9 bits per axis)."""
    g = np.asarray(g, np.uint32)
    m = np.zeros(len(g), np.uint32)
    for i in range(9):
        for a in range(3):
            m |= ((g[:, a] >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + a)
    return m


def query_keys_model(rays, flags=0):
    """keys [n] of svo_ray records: octant mask << 27 | morton27(entry cell) for a valid ray that
    enters the cube (t_min <= t_max), 2^30 - 1 for every other."""
    from raytracingtest_amd.query import sanitize_rays
    F32 = np.float32
    traced, invalid = sanitize_rays(rays, raw=bool(flags & QUERY_RAW))
    o = np.ascontiguousarray(traced["origin"], F32).reshape(-1, 3)
    d = np.ascontiguousarray(traced["dir"], F32).reshape(-1, 3)
    org, _, _, octant, t_min, t_max = ray_setup(o, d)
    g = np.zeros((len(o), 3), np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        enters = ~invalid & (t_min <= t_max)
        for k in range(3):
            e = ((org[k] + t_min * d[:, k]) - F32(1.0)) * F32(512.0)
            e = np.fmin(np.fmax(e, F32(0.0)), F32(511.0))      # NaN -> 0
            g[:, k] = e.astype(np.uint32)                      # in [0, 511]: truncation
    key = (octant.astype(np.uint32) << np.uint32(27)) | morton27(g)
    return np.where(enters, key, np.uint32(KEY_NONE)).astype(np.uint32)


def check_query_keys(keys, index, keys_out, index_out, expected):
    n = len(expected)
    out = []
    for name, b in (("keys", keys), ("index", index), ("keys_out", keys_out), ("index_out", index_out)):
        out += _guard_findings(b, n, name)
    if out:
        return out
    keys, index, keys_out, index_out = (np.asarray(b, np.uint32)[:n] for b in (keys, index, keys_out, index_out))
    bad = np.flatnonzero(keys != expected)
    if len(bad):
        i = int(bad[0])
        out.append(f"{len(bad)} keys differ; ray {i}: {int(keys[i]):#x}, expected {int(expected[i]):#x}")
    if not np.array_equal(index, np.arange(n, dtype=np.uint32)):
        out.append("index is not 0 .. n - 1")
    if np.any(keys_out[1:] < keys_out[:-1]):
        out.append("keys_out decreases")
    if not np.array_equal(np.sort(index_out), np.arange(n, dtype=np.uint32)):
        out.append("index_out is not a permutation")
    elif not np.array_equal(keys_out, keys[index_out]):
        out.append("keys_out[k] != keys[index_out[k]]")
    return out


# ------------------------------------------------------------------ the driver's files
def _u16_blob(a):
    a = np.ascontiguousarray(a, np.uint16)
    if len(a) % 2:
        a = np.concatenate([a, np.zeros(1, np.uint16)])
    return a.view(np.uint32)


def case_tiles(cost, n, with_stats=True):
    return {"kind": 0, "p": [n, int(with_stats)], "blobs": [_u16_blob(cost)], "n": n, "cost": np.asarray(cost, np.uint16),
            "with_stats": with_stats}


def case_strips(cost, n, tiles_x, seg_cap=0, kpack=0, spread=0, part_cost=None, with_stats=True):
    refused = strip_refusal(n, tiles_x, seg_cap, kpack)
    blobs = [_u16_blob(cost)] + ([_u16_blob(part_cost)] if part_cost is not None else [])
    return {"kind": 1, "p": [n, tiles_x, seg_cap, kpack, spread, int(part_cost is not None),
                             HIP_INVALID_VALUE if refused else HIP_SUCCESS, int(with_stats)],
            "blobs": blobs, "n": n, "tiles_x": tiles_x, "seg_cap": seg_cap, "kpack": kpack, "spread": spread,
            "cost": np.asarray(cost, np.uint16), "part_cost": part_cost, "refused": refused, "with_stats": with_stats}


def case_keys(rays, flags=0):
    rays = np.ascontiguousarray(rays)
    assert rays.dtype.itemsize == 32
    return {"kind": 2, "p": [len(rays), flags], "blobs": [rays.view(np.uint32).reshape(-1)], "n": len(rays), "rays": rays,
            "flags": flags}


def write_cases(path, cases):
    words = [np.array([MAGIC, len(cases)], np.uint32)]
    for c in cases:
        p = (list(c["p"]) + [0] * 8)[:8]
        blobs = (list(c["blobs"]) + [np.zeros(0, np.uint32)] * 2)[:2]
        words.append(np.array([c["kind"]] + p + [len(b) for b in blobs], np.int64).astype(np.uint32))
        words += [np.ascontiguousarray(b, np.uint32) for b in blobs]
    np.concatenate(words).astype("<u4").tofile(path)


def read_results(path, n_cases):
    w = np.fromfile(path, "<u4")
    assert w[0] == MAGIC and w[1] == n_cases, "result file: bad header"
    at, out = 2, []
    for _ in range(n_cases):
        kind, err, nb = (int(v) for v in w[at:at + 3])
        at += 3
        blobs = []
        for _ in range(nb):
            ln = int(w[at])
            blobs.append(w[at + 1:at + 1 + ln])
            at += 1 + ln
        out.append({"kind": kind, "err": err, "blobs": blobs})
    assert at == len(w), "result file: trailing words"
    return out
