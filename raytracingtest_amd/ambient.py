"""Ambient rays: the numpy statement of the ambient rule's ray part (csrc/svo_ambient.h,
svo_ambient_rays / svo_set_ambient in include/svo_rt.h; INTEGRATION.md "Ambient").

Direction tables for N in {4, 8, 16}: entry k is (a, b, c) with r = sqrt((k + 0.5) / N),
phi = (k + 0.5) pi (3 - sqrt 5), a = r cos phi, b = r sin phi, c = sqrt(1 - r^2), computed in float64
and rounded once to f32.  The 28 triples committed in csrc/svo_ambient.h are the truth: TABLES is
read from that header's text (float.fromhex of its literals), so the two cannot differ.

From a ray as it was traced (origin o, direction d after the query's clamp) and its hit record, every
operation one f32 rounding:

  1. steps 1-3 of the bounce rule (reflection.entry_face): the entry axis g, out = d_g > 0 ? -1 : +1,
     the origin P off the axis g and face_g + out (side 2^-6) on it
  2. variant v in 0..7: if v & 4 swap a and b, then v & 3 times (a, b) -> (-b, a)        (exact)
  3. direction k: dir_g = out c, dir_{(g+1)%3} = a, dir_{(g+2)%3} = b                     (exact)
  4. the ray {origin, t_max = radius, dir, reserved 0}

A ray is open iff its traced record has neither flag bit 0 (after the t (1 / 64) <= radius filter)
nor bit 4; a hit at t = 0 -- an origin inside a neighbouring voxel -- counts as occluded.
"""
import os
import re

import numpy as np

from ._lib import PKG_DIR
from .query import batch_arrays, sanitize_rays
from .reflection import dead_rays, entry_face

COUNTS = (4, 8, 16)
VARIANTS = 8


def _read_tables():
    text = open(os.path.join(PKG_DIR, "csrc", "svo_ambient.h")).read()
    body = text[text.index("const float T[TABLE_ROWS][3]"):]
    body = body[:body.index("};")]
    rows = re.findall(r"\{\s*(-?0x[0-9a-fA-F.]+p[-+]?\d+)f,\s*(-?0x[0-9a-fA-F.]+p[-+]?\d+)f,\s*(-?0x[0-9a-fA-F.]+p[-+]?\d+)f\s*\}", body)
    if len(rows) != sum(COUNTS):
        raise RuntimeError(f"csrc/svo_ambient.h: {len(rows)} table rows, expected {sum(COUNTS)}")
    vals = np.array([[float.fromhex(v) for v in row] for row in rows], np.float64)
    tab = vals.astype(np.float32)
    if not np.array_equal(tab.astype(np.float64), vals):
        raise RuntimeError("csrc/svo_ambient.h: a table literal is not an f32 number")
    return {n: tab[n - 4:n - 4 + n].copy() for n in COUNTS}


TABLES = _read_tables()   # {N: f32 [N, 3]}


def formula_table(n):
    """The table's definition in float64, rounded once to f32 ([n, 3])."""
    k = np.arange(n, dtype=np.float64) + 0.5
    r = np.sqrt(k / n)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r * r)], axis=1).astype(np.float32)


def variant_table(n, variant):
    """The table of n entries after the variant's swap and quarter turns: f32 [n, 3], exact."""
    if n not in TABLES:
        raise ValueError(f"n_rays must be one of {COUNTS}, got {n}")
    if not 0 <= variant < VARIANTS:
        raise ValueError(f"variant must lie in 0..7, got {variant}")
    t = TABLES[n]
    a, b, c = t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()
    if variant & 4:
        a, b = b, a
    for _ in range(variant & 3):
        a, b = -b, a
    return np.stack([a, b, c], axis=1).astype(np.float32)


def ambient_rays(rays, hits, voxel, n_rays=4, radius=np.inf, variant=0, raw=False):
    """svo_ambient_rays in numpy: out[i * n_rays + k] = ray k of rays[i] (RAY_DTYPE) if hits[i]
    (HIT_DTYPE) has flag bit 0, else the dead ray.  voxel: the hits' voxel keys (uint64).  raw: rays
    were traced with SVO_QUERY_RAW_DIRECTIONS (no small-direction clamp)."""
    f = np.float32
    rays, hits, voxel = batch_arrays(rays, hits, voxel)
    if not (radius > 0):
        raise ValueError(f"radius must be +inf or finite and positive, got {radius}")
    tab = variant_table(n_rays, variant)
    n = len(rays)
    traced, _ = sanitize_rays(rays, raw=raw)
    g, out, org = entry_face(traced["origin"], traced["dir"], hits, voxel)
    a, b, c = tab[None, :, 0], tab[None, :, 1], tab[None, :, 2]
    cg = out[:, None] * c                              # a sign flip
    gg = g[:, None]
    d = np.empty((n, n_rays, 3), f)
    d[:, :, 0] = np.where(gg == 0, cg, np.where(gg == 1, b, a))
    d[:, :, 1] = np.where(gg == 1, cg, np.where(gg == 2, b, a))
    d[:, :, 2] = np.where(gg == 2, cg, np.where(gg == 0, b, a))
    res = dead_rays(n * n_rays).reshape(n, n_rays)
    hit = (hits["flags"] & 1) != 0
    res["origin"][hit] = org[hit][:, None, :]
    res["dir"][hit] = d[hit]
    res["t_max"][hit] = f(radius)
    return res.reshape(-1)
