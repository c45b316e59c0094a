"""The schedule of ppnp_amd/csrc/appnp_dist.hip, pinned on the CPU.

The row-partition engine behind appnp_dist_* holds no kernel.  What it does is request appnp_step*
launches, call the caller's exchange callbacks, and order its two streams with events; a mistake
there is a race or a deadlock between ranks, not a wrong number, and a GPU run with P ranks on one
device would usually survive a missing wait.  tests/native/dist_trace.cpp links the unit's host-only
object (built with -DAPPNP_TESTING) with those of appnp_capi.hip and appnp_propagate.hip against the
recording stand-ins of tests/native/capi_trace.cpp (no HIP runtime, no device), drives every
appnp_dist_* entry point on fabricated row partitions -- failure of each exchange and of each launch
in turn included -- and prints what reaches the device boundary.  The trace must equal
tests/golden/dist_trace.txt byte for byte: the file was recorded from the unit as it stood with four
hand-written loops, before they were folded onto one, and proves the fold requests the same launches,
records and waits in the same stream order.  A change that is meant to alter the schedule
regenerates the file and shows the difference in review.  The sibling test is test_capi_trace.py.
"""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dist_trace.txt")
UNITS = ("appnp_dist", "appnp_capi", "appnp_propagate")


def build(out_dir, dist_source=None):
    """The trace program; dist_source: another appnp_dist.hip to record from (it must sit beside
    the unit's headers)."""
    flags = ["-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-host-only", "-Wall",
             "-Wno-unused-result"]
    csrc = os.path.join(ROOT, "ppnp_amd", "csrc")
    objs = []
    for name in UNITS:
        src = os.path.join(csrc, f"{name}.hip")
        extra = []
        if name == "appnp_dist":
            extra = ["-DAPPNP_TESTING"]  # the APPNP_DIST_TEST_AGREE_FAIL hook
            src = dist_source or src
        objs.append(os.path.join(out_dir, f"{name}.o"))
        subprocess.run([HIPCC, *flags, *extra, "-x", "hip", "-c", src, "-o", objs[-1]], check=True)
    objs.append(os.path.join(out_dir, "dist_trace.o"))
    subprocess.run([HIPCC, *flags, "-x", "hip", "-c",
                    os.path.join(ROOT, "tests", "native", "dist_trace.cpp"), "-o", objs[-1]],
                   check=True)
    exe = os.path.join(out_dir, "dist_trace")
    # linked as plain C++: no HIP runtime, every hip* call resolves to the harness's stand-ins
    subprocess.run(["g++", *objs, "-o", exe, "-lm", "-ldl"], check=True)
    return exe


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    exe = build(str(tmp_path_factory.mktemp("dist_trace")))
    # no APPNP_* variable may reach the units; the program sets the one it drives itself
    r = subprocess.run([exe], env={}, capture_output=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def test_dist_launch_trace_matches_golden(trace):
    with open(GOLDEN, "rb") as fh:
        want = fh.read()
    if trace != want:
        got_lines, want_lines = trace.split(b"\n"), want.split(b"\n")
        case = b""
        for i, (a, b) in enumerate(zip(got_lines, want_lines)):
            if b.startswith(b"# "):
                case = b
            if a != b:
                raise AssertionError(
                    f"trace differs at line {i + 1}, case {case.decode()!r}:\n"
                    f"  got  {a.decode()}\n  want {b.decode()}")
        raise AssertionError(f"trace has {len(got_lines)} lines, golden {len(want_lines)}")


def test_golden_is_no_larger_than_its_sibling():
    assert os.path.getsize(GOLDEN) <= 303013  # tests/golden/capi_trace.txt when this was recorded


def test_rejected_calls_request_nothing(trace):
    inside, seen = False, 0
    for line in trace.decode().split("\n"):
        if line == "rejected-begin":
            assert not inside
            inside = True
        elif line == "rejected-end":
            assert inside
            inside = False
        elif inside:
            # a launch, a copy, an event, a wait or an exchange would print a line of its own
            m = re.fullmatch(r"rc (.+) -> (-?\d+)", line)
            assert m, line
            seen += 1
    assert not inside and seen >= 40


def test_pipeline_groups_equal_the_python_shard_groups(trace):
    from ppnp_amd.dist import shard_groups

    got = {}
    # one line per R: the groups of rank 0, 1, ... separated by blanks, "lo-hi,lo-hi" each
    for m in re.finditer(rb"^pipeline_groups R=(\d+):((?: \d+-\d+(?:,\d+-\d+)*)*)$", trace, re.M):
        for ri, groups in enumerate(m.group(2).split()):
            got[(int(m.group(1)), ri)] = [tuple(int(v) for v in g.split(b"-"))
                                          for g in groups.split(b",")]
    want = {(R, ri): [tuple(g) for g in shard_groups(R, ri)]
            for R in range(3, 18) for ri in range(R)}
    assert got == want
