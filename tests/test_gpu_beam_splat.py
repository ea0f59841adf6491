"""beam_splat_kernel on the GPU against its model (tests/beam_model.py splat_model).  A tile
bound that is too low leaves every frame bit-identical and only costs time, and one that is too high shows in
a frame only if a ray happens to hit inside the margin -- so no parity test pins the entries.  Here every word
the splat writes is compared: with E the bound a reader of a tile takes (the min of its tile's, its super
tile's and the global word, another generation's reading as +inf),

  safety      E <= hi_geo (1 + 2^-21) + 2^-23 sum_k (|rel_k| + size)   pure float64 geometry: beam_start's premise
  rule, upper E <= hi_rule (1 + 2^-21)                                  every box reaches the tiles its rule names
  rule, lower E >= lo_rule (1 - 2^-21), +inf where nothing reaches      and no others: tightness
  structure   high halves ~gen or all-ones, the guard words, no word of a level no box can take, exactly

One process does all the GPU work: tests/beam_splat_driver.cpp (host code only) runs every case of
tests/beam_cases.py on one stream and writes one result file.  The tests below only compare."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import beam_cases as bc
from tests import beam_model as bm
from tests.test_beam_model import build_driver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(cases, per case the buffers after each step) of the one driver run; a driver that exits non-zero or by
    a signal fails the fixture, and with it every test of the module, with the driver's output."""
    d = tmp_path_factory.mktemp("beam_splat")
    exe = build_driver(d)
    cases = bc.all_cases()
    bm.write_cases(d / "cases.bin", cases)
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True,
                         timeout=120)
    if out.returncode != 0:
        pytest.fail(f"beam_splat_driver exited with {out.returncode}: {out.stdout[-1000:]}{out.stderr[-3000:]}")
    return cases, bm.read_results(d / "results.bin", cases)


def _E(buf, bp, gen):
    n = bm.buffer_words(bp)
    assert len(buf) == 2 * n + bm.GUARD_WORDS
    return bm.decode(np.ascontiguousarray(buf[:2 * n]).view(np.uint64), bp, gen)[0]


def _report(findings, ran):
    assert ran > 0
    assert not findings, f"{len(findings)} of {ran} cases disagree with the model:\n" + \
        "\n".join(f"{name}: {'; '.join(f[:3])}" for name, f in findings[:20])


def test_safety_and_rule_envelope(run):
    """Every tile of every case (the buffer after the case's last step, read at that step's generation)."""
    models = bc.models()
    findings, worst = [], {}
    for c, bufs in zip(*run):
        gen, bp = c["steps"][-1]
        m = models[c["name"]]
        E = _E(bufs[-1], bp, gen)
        f = bm.check_envelope(E, m)
        if f:
            findings.append((c["name"], f))
        pinned = np.isfinite(m["hi_rule"]) & (m["hi_rule"] == m["lo_rule"]) & (m["hi_rule"] > 0.0) & np.isfinite(E)
        if pinned.any():
            worst[c["name"]] = float(np.max(np.abs(E[pinned] / m["hi_rule"][pinned] - 1.0)))
    top = max(worst.values())
    print(f"beam splat: largest |E / d_rule - 1| over the pinned tiles {top:.3e} = {top * 2.0 ** 24:.2f} x 2^-24 "
          f"(tolerance 2^-21), in {max(worst, key=worst.get)!r}")
    if os.environ.get("SVO_BEAM_SPLAT_OUT"):
        with open(os.environ["SVO_BEAM_SPLAT_OUT"], "w") as fh:
            json.dump({"largest_rel_dev": top, "tolerance": bm.REL, "case": max(worst, key=worst.get), "per_case": worst},
                      fh, indent=1)
    _report(findings, len(run[0]))


def test_structure(run):
    """The first step of every case starts from an all-ones buffer: high halves ~gen or all-ones, guard words
    intact, no tile word outside every outer rectangle, no super word without a box that can be kind 2, no global
    word without one that can be kind 3."""
    models = bc.models()
    findings = []
    for c, bufs in zip(*run):
        gen, bp = c["steps"][0]
        m = models[c["name"]] if len(c["steps"]) == 1 else bm.splat_model(bp, c["boxes"])
        f = bm.check_structure(bufs[0], bp, gen, m)
        if f:
            findings.append((c["name"], f))
    _report(findings, len(run[0]))


def test_no_boxes_no_launch(run):
    got = {c["name"]: b for c, b in zip(*run)}["boxes n=0"][0]
    assert np.all(got[:-bm.GUARD_WORDS] == 0xFFFFFFFF) and np.all(got[-bm.GUARD_WORDS:] == bm.GUARD)


def test_window_and_global_atomics_agree(run):
    """The two corner boxes leave the same tile words whether the workgroup's rectangle fits the LDS window
    (8192 tiles) or not (8256: global atomics): in tile coordinates their tiles are the frames' corners."""
    got = {c["name"]: (c, b) for c, b in zip(*run)}
    grids = []
    for w in (1024, 1032):
        c, bufs = got[f"window {w}x512 corners"]
        bp = c["bp"]
        E = _E(bufs[0], bp, bp["gen"]).reshape(bp["tiles_y"], bp["tiles_x"])
        assert np.isfinite(E).sum() == 18                      # 3 x 3 tiles in each corner
        grids.append((E[:3, :3], E[-3:, -3:]))
    assert np.array_equal(grids[0][0], grids[1][0]) and np.array_equal(grids[0][1], grids[1][1])


def test_generations(run):
    """Generation 1 with camera A, then 2 with camera B on the same buffer, against 2 on a fresh one: every word
    the fresh run wrote is equal in the reused buffer (a min over a set has no order), every other word is
    all-ones or still carries generation 1 (~1 in its high half)."""
    got = {c["name"]: (c, b) for c, b in zip(*run)}
    c, (first, reused) = got["generations: 1 then 2"]
    _, (fresh,) = got["generations: 2 fresh"]
    n = bm.buffer_words(c["bp"])
    first, reused, fresh = (np.ascontiguousarray(b[:2 * n]).view(np.uint64) for b in (first, reused, fresh))
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    wrote = fresh != ones
    assert wrote.sum() > 100
    assert np.array_equal(reused[wrote], fresh[wrote])
    rest = reused[~wrote]
    assert np.all((rest == ones) | ((rest >> np.uint64(32)) == np.uint64(0xFFFFFFFE)))
    assert np.array_equal(rest, first[~wrote])                 # ... and is what generation 1 left there
    assert np.any((rest >> np.uint64(32)) == np.uint64(0xFFFFFFFE))
    # the ends of the generation range: the same distances under another high half
    _, (lo_gen,) = got["generation 1"]
    _, (hi_gen,) = got["generation 0xFFFFFFFE"]
    lo_gen, hi_gen = (np.ascontiguousarray(b[:2 * n]).view(np.uint64) for b in (lo_gen, hi_gen))
    w = lo_gen != ones
    assert np.array_equal(w, hi_gen != ones)
    assert np.all(lo_gen[w] >> np.uint64(32) == np.uint64(0xFFFFFFFE)) and np.all(hi_gen[w] >> np.uint64(32) == np.uint64(1))
    assert np.array_equal(lo_gen[w] & np.uint64(0xFFFFFFFF), hi_gen[w] & np.uint64(0xFFFFFFFF))
