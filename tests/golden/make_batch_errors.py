"""Record tests/golden/batch_errors.json: (return code, svo_last_error text) of every call in
tests/batch_error_cases.py, from the library this is run against.

    python tests/golden/make_batch_errors.py [path/to/libsvo_rt.so]

The recording is the behaviour to keep, so run it against a build of the commit BEFORE a change to the entry
points (build that commit, or name its library), never against the code under test.  No call reaches a device.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
if len(sys.argv) > 1:
    os.environ["SVO_RT_LIB"] = os.path.abspath(sys.argv[1])

from raytracingtest_amd import _lib            # noqa: E402
from tests import batch_error_cases as cases   # noqa: E402


def main():
    m = cases.Memory()
    rows = cases.run(_lib.lib(), m)
    assert m.unwritten(), "a call wrote to the context or to a caller array"
    out = os.path.join(ROOT, "tests", "golden", "batch_errors.json")
    with open(out, "w") as fh:
        json.dump({"abi_version": _lib.lib().svo_abi_version(),
                   "cases": [{"id": i, "rc": rc, "error": msg} for i, rc, msg in rows]}, fh, indent=1)
        fh.write("\n")
    print(f"{len(rows)} cases -> {out}")


if __name__ == "__main__":
    main()
