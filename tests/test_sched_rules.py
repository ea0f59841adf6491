"""The launch scheduling rules (raytracingtest_amd/csrc/svo_sched.h: loop form, class table, choice
of the built order, order refresh) on a CPU: tests/sched_rules_driver.cpp, a plain C++ program that
includes only that header, evaluates the table below and prints one result line per case.  Every
expectation is worked out by hand from the rule's text (the arithmetic stands beside the case);
boundary cases use powers of two for the ratio and the slots, so their products are exact, and every
other case lies some percent off its threshold.  The same driver runs once more under
AddressSanitizer + UndefinedBehaviorSanitizer, as a process of its own."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

GXX = shutil.which("g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]

# loop T M slots ratio thin_ratio seg_min_chain prior prior_lat -> lat is_short thin
# ratio 0.25 x slots 8192 x M 100 = 204800 exactly; thin 0.0625 x 8192 x 100 = 51200 exactly
LOOP = [
    ("loop 204799 100 8192 0.25 0.0625 160 0 0", "1 1 0"),   # no prior: below the threshold
    ("loop 204800 100 8192 0.25 0.0625 160 0 0", "0 1 0"),   # ... on it: strict <, lean
    # a prior latency decision: bound 0.25 x 1.15 = 0.2875, threshold 235520
    ("loop 225280 100 8192 0.25 0.0625 160 1 1", "1 1 0"),   # 1.10 x 204800 stays latency
    ("loop 245760 100 8192 0.25 0.0625 160 1 1", "0 1 0"),   # 1.20 x drops to lean
    # a prior lean decision: bound 0.25 / 1.15 = 0.21739, threshold 178087
    ("loop 184320 100 8192 0.25 0.0625 160 1 0", "0 1 0"),   # 0.90 x stays lean
    ("loop 163840 100 8192 0.25 0.0625 160 1 0", "1 1 0"),   # 0.80 x flips to latency
    ("loop 225280 100 8192 0.25 0.0625 160 0 1", "0 1 0"),   # prior_lat means nothing without a prior
    ("loop 0 0 8192 0.25 0.0625 160 0 0", "0 1 0"),          # M = 0: lean whatever T is
    ("loop 5 0 8192 0.25 0.0625 160 1 1", "0 1 0"),
    # is_short on both sides of seg_min_chain (T far above 0.25 x 8192 x 160 = 327680: lean)
    ("loop 1000000000 159 8192 0.25 0.0625 160 0 0", "0 1 0"),
    ("loop 1000000000 160 8192 0.25 0.0625 160 0 0", "0 0 0"),
    ("loop 1000 160 8192 0.25 0.0625 160 0 0", "1 0 1"),
    ("loop 51199 100 8192 0.25 0.0625 160 0 0", "1 1 1"),    # thin: below 51200
    ("loop 51200 100 8192 0.25 0.0625 160 0 0", "1 1 0"),    # ... on it: not thin
    # thin only with lat: thin_ratio 0.5 (threshold 409600) above the ratio
    ("loop 204800 100 8192 0.25 0.5 160 0 0", "0 1 0"),
    ("loop 204799 100 8192 0.25 0.5 160 0 0", "1 1 1"),
    # thin has no hysteresis: prior latency keeps lat at 225280, thin still by 51200
    ("loop 51200 100 8192 0.25 0.0625 160 1 1", "1 1 0"),
]
# slots num_cus lds_bytes: 163840 / 4608 = 35 -> at most 32 per CU; 163840 / 16384 = 10
SLOTS = [("slots 256 4608", "8192"), ("slots 256 16384", "2560"), ("slots 256 5120", "8192"), ("slots 256 5632", "7424")]
# stats: 8 x (max, sum) words; M = the largest even word, T = the sum of the odd ones (past 2^32)
STATS = [
    ("stats 5 1000 90 2000 17 3000 3 4000 260 5000 41 6000 8 7000 77 4000000000", "4000028000 260"),
    ("stats 0 0 0 0 0 0 0 0 0 0 0 0 0 0 9 1", "1 9"),
]
# class seg_all seg_cap latency_bound lat_short lat_thin jittered seg_jitter kpack_lat kpack_issue kpack_thin -> kpack seg
# (tables 0x444 = 1092, 0x4 = 4, 0x888 = 2184; 2 x 0x111111 = 0x222222 = 2236962)
CLASS = [
    ("class 2 96 1 1 0 0 2 1092 4 2184", "2236962 96"),   # seg_all: its own table whatever the decision
    ("class 2 0 1 1 0 0 2 1092 4 2184", "0 0"),           # ... but no segments without a seg_cap
    ("class 0 96 1 1 0 0 2 1092 4 2184", "0 0"),          # latency-bound with short chains
    ("class 0 96 0 1 1 0 2 1092 4 2184", "4 96"),         # short / thin mean nothing when issue-bound
    ("class 0 96 1 0 0 1 0 1092 4 2184", "0 0"),          # jittered with seg_jitter 0
    ("class 0 96 1 0 0 1 2 1092 4 2184", "1092 96"),      # jittered otherwise: the decision's table
    ("class 0 96 1 0 1 0 2 1092 4 2184", "2184 96"),      # latency, thin
    ("class 0 96 1 0 0 0 2 1092 4 2184", "1092 96"),      # latency
    ("class 0 96 0 0 0 0 2 1092 4 2184", "4 96"),         # issue
    ("class 0 0 1 0 0 0 2 1092 4 2184", "0 0"),           # seg_cap 0
    ("class 0 96 0 0 0 0 2 1092 0 2184", "0 0"),          # an empty table: no segments
]
# pick n build_at0 build_at1 build_key0 build_key1 okey key -> use; keys width/seg/kpack.
# n = 5: eligible are builds at 0 .. 3
A, K = "640/96/1092", "640/0/0"
PICK = [
    (f"pick 5 3 4 {A} {A} {A} {K}", "0"),                  # slot 1 too new
    (f"pick 5 4 3 {A} {A} {A} {K}", "1"),
    (f"pick 5 2 3 {A} {A} {A} {K}", "1"),                  # equal keys: the newer
    (f"pick 5 3 2 {A} {A} {A} {K}", "0"),
    (f"pick 5 2 3 {A} 640/96/4 {A} {K}", "0"),             # the exact key beats a newer build of another table
    (f"pick 5 2 3 640/96/4 640/0/0 {A} {K}", "1"),         # no exact key: the newest at the geometry
    (f"pick 5 2 3 640/96/4 800/0/0 {A} {K}", "0"),
    (f"pick 5 2 4 640/96/4 640/0/0 {A} {K}", "0"),         # ... among the eligible
    (f"pick 5 2 3 800/96/1092 800/0/0 {A} {K}", "-1"),     # another geometry
    (f"pick 5 2 3 640/96/4 {A} {K} {K}", "-1"),            # no segmented order for an unsegmented launch
    (f"pick 5 1 3 {K} 640/96/4 {K} {K}", "0"),
    (f"pick 5 4 5 {A} {A} {A} {K}", "-1"),                 # nothing eligible
    (f"pick 5 -1 -1 {A} {A} {A} {K}", "-1"),
    (f"pick 1 -1 -1 {A} {A} {A} {K}", "-1"),               # n - 2 = -1: a slot never built stays out
    (f"pick 5 -1 3 {A} {A} {A} {K}", "1"),
]
# layout enabled has_order seg kmax used_kpack okey_seg okey_kmax okey_kpack -> ran in another class layout
LAYOUT = [
    ("layout 1 1 96 4 1092 96 4 1092", "0"),
    ("layout 1 1 0 1 0 96 4 1092", "1"),       # an unsegmented order for a segmenting launch
    ("layout 1 1 96 8 1092 96 4 1092", "1"),   # another kmax
    ("layout 1 1 96 4 4 96 4 1092", "1"),      # another table
    ("layout 1 1 0 8 0 0 4 0", "0"),           # kmax counts only where the launch segments
    ("layout 0 1 0 1 0 96 4 1092", "0"),       # switched off
    ("layout 1 0 0 1 0 96 4 1092", "0"),       # no order taken
]
# refresh key_changed n order_every drift mode_changed own_layout held_splat view_changed moving since_build move_every
REFRESH = [
    ("refresh 0 5 32 0 0 0 0 0 0 0 4", "0"),
    ("refresh 1 5 32 0 0 0 0 0 0 0 4", "1"),
    ("refresh 0 64 32 1 0 0 0 0 0 0 4", "1"),   # the periodic rebuild ...
    ("refresh 0 0 32 1 0 0 0 0 0 0 4", "1"),
    ("refresh 0 64 32 0 0 0 0 0 0 0 4", "0"),   # ... only with drift
    ("refresh 0 65 32 1 0 0 0 0 0 0 4", "0"),   # ... and only every order_every-th launch
    ("refresh 0 5 32 0 1 0 0 0 0 0 4", "1"),
    ("refresh 0 5 32 0 0 1 0 0 0 0 4", "1"),
    ("refresh 0 5 32 0 0 0 1 0 0 0 4", "1"),
    ("refresh 0 5 32 0 0 0 0 1 0 0 4", "1"),    # a new view the camera holds: at once
    ("refresh 0 5 32 0 0 0 0 1 1 3 4", "0"),    # a moving camera: every move_every-th launch
    ("refresh 0 5 32 0 0 0 0 1 1 4 4", "1"),
    ("refresh 0 5 32 0 0 0 0 0 1 10 4", "0"),   # moving alone (the order is this view's already)
]
CASES = LOOP + SLOTS + STATS + CLASS + PICK + LAYOUT + REFRESH


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    if GXX is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("sched")
    out = {}
    for name, flags in (("plain", []), ("asan_ubsan", SAN)):
        exe = str(d / f"sched_{name}")
        cmd = [GXX, "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", os.path.join(ROOT, "raytracingtest_amd", "csrc"),
               os.path.join(ROOT, "tests", "sched_rules_driver.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        out[name] = (exe if r.returncode == 0 else None, r.stderr)
    return out


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_rules(builds, build):
    exe, err = builds[build]
    if exe is None:
        assert build != "plain", err[-2000:]
        pytest.skip(f"{build} toolchain unavailable: {err[-400:]}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="".join(c + "\n" for c, _ in CASES), capture_output=True, text=True, env=env,
                       timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-400:], r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(CASES)
    wrong = [(c, want, g) for (c, want), g in zip(CASES, got) if g != want]
    assert not wrong, wrong


def test_header_stands_alone():
    """The rules need no HIP: the header includes nothing but <algorithm> and <cstdint>."""
    with open(os.path.join(ROOT, "raytracingtest_amd", "csrc", "svo_sched.h")) as f:
        inc = sorted(ln.split()[1] for ln in f if ln.startswith("#include"))
    assert inc == ["<algorithm>", "<cstdint>"]
