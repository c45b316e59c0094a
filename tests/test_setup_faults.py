"""Every failure point of the set-up builders, taken on the CPU.

graph_build, build_heavy, graph_build_shard_offsets, graph_build_source_blocks,
graph_build_transpose, standardize and csr_transpose allocate, launch, read a count back and
allocate again.  tests/native/setup_faults.cpp links their three units (compiled as usual, device
code included, so nothing of them is left out) against stand-ins for the HIP runtime that track
every allocation and can fail any hipMalloc or hipStreamSynchronize.  It fails every allocation
and every synchronisation of every driver in turn, none sampled, and checks the return code, that
nothing is live after the clean-up the public entry point performs, that nothing was freed twice,
and, for the best-effort source-block builder, that the last-error slot is clear and the graph is
left as found.  No device is touched.
"""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "ppnp_amd", "csrc")
UNITS = ["appnp_graph", "appnp_blocks", "appnp_ingest"]
# one line per driver: (name, allocations, synchronisations) of its clean run.  A builder that
# takes one allocation more or fewer changes its line here, on purpose and in review.
DRIVERS = [
    ("build_heavy", 5, 2),
    ("graph_build", 18, 6),
    ("graph_build split", 26, 6),
    ("shard_offsets first", 1, 1),
    ("shard_offsets replacing", 1, 1),
    ("source_blocks unit sym w4", 8, 2),
    ("source_blocks unit sym w16", 8, 2),
    ("source_blocks weighted sym w4", 7, 2),
    ("source_blocks weighted sym w16", 7, 2),
    ("source_blocks unit rw w4", 7, 2),
    ("source_blocks unit rw w16", 7, 2),
    ("source_blocks weighted rw w4", 7, 2),
    ("source_blocks weighted rw w16", 7, 2),
    ("source_blocks unit sym held rows", 8, 2),
    ("graph_build_transpose", 17, 5),
    ("standardize", 17, 4),
    ("standardize lcc", 17, 5),
    ("csr_transpose", 6, 1),
    ("csr_transpose values", 7, 1),
]


def build(out_dir):
    flags = ["-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result"]
    objs = [os.path.join(out_dir, u + ".o") for u in UNITS]
    harness = os.path.join(out_dir, "setup_faults.o")
    exe = os.path.join(out_dir, "setup_faults")
    # the product units, exactly as the library compiles them but for -O1; the harness host-only
    jobs = [subprocess.Popen([HIPCC, *flags, "-c", os.path.join(CSRC, u + ".hip"), "-o", o])
            for u, o in zip(UNITS, objs)]
    jobs.append(subprocess.Popen([HIPCC, *flags, "--cuda-host-only", "-x", "hip", "-c",
                                  os.path.join(ROOT, "tests", "native", "setup_faults.cpp"),
                                  "-o", harness]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    # linked as plain C++: no HIP runtime, every hip* call resolves to the harness's stand-ins
    subprocess.run(["g++", *objs, harness, "-o", exe, "-lm"], check=True)
    return exe


def test_setup_builders_survive_every_failed_allocation_and_sync(tmp_path):
    exe = build(str(tmp_path))
    r = subprocess.run([exe], env={}, capture_output=True, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-2000:]
    lines = out.strip().split("\n")
    assert lines[-1] == "all clean", out[-4000:]
    got = []
    for line in lines[:-1]:
        name, rest = line.split(" allocs ")
        allocs, rest = rest.split(" syncs ")
        syncs, verdict = rest.split()
        assert verdict == "ok", line
        got.append((name.strip(), int(allocs), int(syncs)))
    assert got == DRIVERS
