"""The placement-only kernels on the GPU against their models (tests/placement_model.py): the tile
order, the strip order with segmented tiles and the ordered queries' keys and sort.  Whatever these
kernels write, frames and ray batches come out bit-identical -- only their time changes -- so no
parity test sees them; here every word they write is compared, and the 64 guard words behind every
buffer too.

One process does all the GPU work: tests/placement_driver.cpp (host code only) reads every case of
tests/placement_cases.py from one file, runs them on one stream and writes one result file.  The
tests below only compare that file with the models.  Every comparison is exact integer equality."""
import subprocess

import numpy as np
import pytest

from tests import placement_cases as pc
from tests import placement_model as pm
from tests.test_placement_model import build_driver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(cases, results) of the one driver run; a driver that exits non-zero or by a signal fails the fixture,
    and with it every test of the module, with the driver's output."""
    d = tmp_path_factory.mktemp("placement")
    exe = build_driver(d)
    cases = pc.all_cases()
    pm.write_cases(d / "cases.bin", [c for _, c in cases])
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True,
                         timeout=120)
    if out.returncode != 0:
        pytest.fail(f"placement_driver exited with {out.returncode}: {out.stdout[-1000:]}{out.stderr[-3000:]}")
    results = pm.read_results(d / "results.bin", len(cases))
    assert [r["kind"] for r in results] == [c["kind"] for _, c in cases]
    return cases, results


def _report(findings, ran):
    assert ran > 0
    assert not findings, f"{len(findings)} of {ran} cases disagree with the model:\n" + \
        "\n".join(f"{name}: {'; '.join(f[:3])}" for name, f in findings[:20])


def test_tile_order(run):
    findings, ran = [], 0
    for (name, c), r in zip(*run):
        if c["kind"] != 0:
            continue
        ran += 1
        order, stats = r["blobs"]
        f = [] if r["err"] == pm.HIP_SUCCESS else [f"hipError {r['err']}"]
        f += pm.check_tile_order(order, stats, pm.tile_order_model(c["cost"], c["n"]), c["with_stats"])
        if f:
            findings.append((name, f))
    assert ran == len(pc.tile_cases()) + len(pc.repeat_cases())
    _report(findings, ran)


def test_tile_order_repeats_bit_identically(run):
    """No atomics in the tile order: the same input twice gives the same bytes, the free order included."""
    got = {name: r for (name, _), r in zip(*run) if "repeat" in name}
    assert len(got) == 4
    for n in (2047, 70001):
        a, b = got[f"tiles n={n} repeat 0"], got[f"tiles n={n} repeat 1"]
        assert all(np.array_equal(x, y) for x, y in zip(a["blobs"], b["blobs"])), n


def test_strip_order(run):
    """Per XCD and class: the block's start and end, the segmented groups' count, place and part codes, the
    plain entries, each tile of the class exactly once; the padding, the class ends, the statistics, the
    guard words.  Unchecked, because an LDS atomic decides it: WHICH tiles of a class are the segmented ones."""
    findings, ran = [], 0
    for (name, c), r in zip(*run):
        if c["kind"] != 1 or c["refused"]:
            continue
        ran += 1
        order, stats = r["blobs"]
        m = pm.strip_order_model(c["cost"], c["n"], c["tiles_x"], c["seg_cap"], c["kpack"], c["spread"], c["part_cost"])
        f = [] if r["err"] == pm.HIP_SUCCESS else [f"hipError {r['err']}"]
        f += pm.check_strip_order(order, stats, m, c["with_stats"])
        if f:
            findings.append((name, f))
    assert ran == len(pc.strip_cases())
    _report(findings, ran)


def test_strip_order_refusals(run):
    """A kpack nibble outside {0, 4, 8}, seg_cap > 0 with n no multiple of tiles_x, a grid of 2^28:
    hipErrorInvalidValue, no launch, the buffers untouched."""
    ran = 0
    for (name, c), r in zip(*run):
        if c["kind"] == 1 and c["refused"]:
            ran += 1
            assert r["err"] == pm.HIP_INVALID_VALUE, name
            assert all(pm.untouched(b) for b in r["blobs"]), name
    assert ran == 4


def test_query_keys_and_sort(run):
    """Every ray's key equals the model's (none is excluded), index[i] = i; behind the sort keys_out is
    non-decreasing, index_out a permutation and keys_out[k] = keys[index_out[k]]."""
    findings, ran = [], 0
    for (name, c), r in zip(*run):
        if c["kind"] != 2:
            continue
        ran += 1
        f = pm.check_query_keys(*r["blobs"], pm.query_keys_model(c["rays"], c["flags"]))
        if f:
            findings.append((name, f))
    assert ran == len(pc.query_cases())
    _report(findings, ran)
