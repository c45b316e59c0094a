"""The launch sequence of ppnp_amd/csrc/appnp_capi.hip and appnp_propagate.hip, pinned on the CPU.

Those units hold no kernel: their whole observable behaviour is the launches they request from
the other units, the arguments of each, and their return codes.  tests/native/capi_trace.cpp links
their host-only objects against recording stand-ins (for their internal imports and for the HIP
runtime calls they make -- the HIP runtime itself is not linked, so no device is ever touched),
drives every public entry point on fabricated graphs, and prints the trace.  The trace must equal
tests/golden/capi_trace.txt byte for byte: the file was recorded before the orchestration was
folded onto shared helpers and is the proof that a change to the units requests the same launches
(the appnp_poly cases were recorded before the propagation calls got a unit of their own).
A change that is meant to alter a launch regenerates the file and shows the difference in review.
The row-partition engine (appnp_dist.hip) is pinned the same way by the sibling test_dist_trace.py;
the two programs share the stand-ins of capi_trace.cpp.
"""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_trace.txt")
UNITS = ("appnp_capi", "appnp_propagate")


def build(out_dir):
    flags = ["-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-host-only", "-Wall",
             "-Wno-unused-result"]
    units = [os.path.join(out_dir, f"{name}.o") for name in UNITS]
    harness = os.path.join(out_dir, "capi_trace.o")
    exe = os.path.join(out_dir, "capi_trace")
    for name, unit in zip(UNITS, units):
        subprocess.run([HIPCC, *flags, "-c", os.path.join(ROOT, "ppnp_amd", "csrc", f"{name}.hip"),
                        "-o", unit], check=True)
    subprocess.run([HIPCC, *flags, "-x", "hip", "-c",
                    os.path.join(ROOT, "tests", "native", "capi_trace.cpp"), "-o", harness],
                   check=True)
    # linked as plain C++: no HIP runtime, every hip* call resolves to the harness's stand-ins
    subprocess.run(["g++", *units, harness, "-o", exe, "-lm"], check=True)
    return exe


def test_capi_launch_trace_matches_golden(tmp_path):
    exe = build(str(tmp_path))
    # no APPNP_* override may reach the units (they cache them), and nothing else is needed
    r = subprocess.run([exe], env={}, capture_output=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    with open(GOLDEN, "rb") as fh:
        want = fh.read()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.split(b"\n"), want.split(b"\n")
        case = b""
        for i, (a, b) in enumerate(zip(got_lines, want_lines)):
            if b.startswith(b"# "):
                case = b
            if a != b:
                raise AssertionError(
                    f"trace differs at line {i + 1}, case {case.decode()!r}:\n"
                    f"  got  {a.decode()}\n  want {b.decode()}")
        raise AssertionError(f"trace has {len(got_lines)} lines, golden {len(want_lines)}")
