"""CPU: the roofline block bench.py prints is self-consistent for every kind of iteration the
runs take -- one GPU with split rows, a narrow 8-rank column slab that runs wholly in the
remainder pass, a row-layout rank with an exchange, and a graph with gather locality.

The ceiling is a lower bound on the iteration time, so ``ceiling.frac >= frac`` always (the
round-2 rehearsal line reported a ceiling from the streams alone, with 0 lines per nonzero).
No GPU: ``bench.roofline`` is plain arithmetic on the shape and the measured time."""

import os

import pytest

import bench

N, NNZ, F = 2_449_029, 126_165_965, 100


def _check(rl, measured_ms):
    assert rl["avg_launch_ms"] == measured_ms
    assert 0 < rl["frac"] <= rl["ceiling"]["frac"] <= 1.0 + 1e-12
    assert rl["ceiling"]["ms_per_iter"] <= measured_ms
    assert rl["achieved"] == pytest.approx(rl["bytes_per_launch"] / (measured_ms * 1e-3) / 1e9)
    return rl


def test_single_gpu_split_rows():
    rl = _check(bench.roofline(n=N, rows=N, nnz=NNZ, F_local=F, esz=4, avg_iter_ms=7.79, fs=96,
                               r=4, lpe=1), 7.79)
    # B_iter = 4(N+1) + 8 nnz + 3 N F s on one GPU
    assert rl["bytes_per_launch"] == 4 * (N + 1) + 8 * NNZ + 3 * N * F * 4
    assert rl["ceiling"]["lines_per_nonzero"] == 3
    assert rl["ceiling"]["remainder_l2_requests_per_nonzero"] == 1
    assert 0.06 < rl["frac"] < 0.07 and rl["ceiling"]["frac"] < 0.08
    assert not rl["ceiling"]["clamped_to_measured"]


def test_whole_rows_count_four_lines():
    rl = _check(bench.roofline(n=N, rows=N, nnz=NNZ, F_local=F, esz=4, avg_iter_ms=9.57, fs=F,
                               r=0, lpe=1), 9.57)
    assert rl["ceiling"]["lines_per_nonzero"] == 4  # a 400-B packed row spans 4 lines


# measured times of the remainder pass on products-synth's shape (126.2 M nonzeros unless noted)
W16_COL8_MS = 1.776                     # the 8-rank column slab's W16 pass (profiles/r4p_col8_*)
W16_PROBE_MS, W16_PROBE_NNZ = 1.894, 127_349_508  # profiles/r2_blk_probe.txt


def test_narrow_column_slab_in_the_remainder_pass():
    """13 of 100 columns on 8 ranks: no direct gather (0 lines per nonzero), the W16 pass.  The
    ceiling prices the pass from counts: its L2 fill per row pass (4 passes x 8
    XCDs x the 157 MB table) and its L2 requests -- not its own measured time, which made round
    4's ceiling certify the kernel against itself -- so it sits well below the measured 1.776 ms."""
    rl = _check(bench.roofline(n=N, rows=N, nnz=NNZ, F_local=13, esz=4,
                               avg_iter_ms=W16_COL8_MS, fs=0, r=13, lpe=4), W16_COL8_MS)
    assert rl["ceiling"]["lines_per_nonzero"] == 0
    assert rl["ceiling"]["remainder_l2_requests_per_nonzero"] == 4
    assert rl["bytes_per_launch"] == 4 * (N + 1) + 8 * NNZ + 3 * N * 13 * 4
    c = rl["ceiling"]
    assert c["ms_per_iter"] <= 0.9 * W16_COL8_MS
    assert c["ms_per_iter"] >= c["hbm_ms"]
    fl = c["remainder_pass_floor"]
    assert fl["row_passes"] == 4 and fl["fill_lines"] == 4 * 8 * N * 64 / 128
    assert "count floor" in fl["kind"]
    assert 0.2 < rl["ceiling"]["frac"] < 0.3  # 1.40 GB in >= 0.72 ms


@pytest.mark.parametrize("lpe,nnz,measured_ms,passes", [
    (1, W16_PROBE_NNZ, 0.680, 1),  # W4: the probe (profiles/r2_blk_probe.txt)
    (1, NNZ, 0.766, 1),            # W4: the library's pass (profiles/r4_driver_cmd_kernel_stats)
    (2, NNZ, 1.105, 2),            # W8: F = 40's pass, barrier every 32 blocks (r4_sync_ab)
    (4, NNZ, 1.769, 4),            # W16: the 13-column slab's pass, same (r4_sync_ab)
    (4, W16_PROBE_NNZ, W16_PROBE_MS, 4)])
def test_remainder_floor_is_below_every_measurement(lpe, nnz, measured_ms, passes):
    """Every width of the pass: the count floor is at most every time measured for it, and its
    row passes are the library's (graph_build_source_blocks: 640 / LPE rows per wave group, 16
    waves on each of 256 CUs)."""
    fl = bench.remainder_floor(N, N, nnz, lpe)
    assert fl["row_passes"] == passes
    assert fl["ms"] <= measured_ms
    assert fl["ms"] == max(fl["fill_ms"], fl["l2_request_ms"])
    rl = bench.roofline(n=N, rows=N, nnz=nnz, F_local=4 * lpe, esz=4,
                        avg_iter_ms=10.0, fs=0, r=4 * lpe, lpe=lpe)
    assert rl["ceiling"]["remainder_pass_ms"] == fl["ms"]


def test_row_layout_rank_with_exchange():
    rows, nnz = -(-N // 8), NNZ // 8
    ex = 7 * rows * F * 4
    rl = _check(bench.roofline(n=N, rows=rows, nnz=nnz, F_local=F, esz=4, avg_iter_ms=2.5,
                               fs=F, r=0, lpe=1, exchange_in_bytes=ex), 2.5)
    # the rank reads all n rows of Z_k (gathered), its own H rows and writes its Z rows
    assert rl["bytes_per_launch"] == 4 * (rows + 1) + 8 * nnz + (N + 2 * rows) * F * 4
    c = rl["ceiling"]
    assert c["exchange_in_bytes"] == ex and c["exchange_ms"] > c["compute_ms"]
    assert c["ms_per_iter"] == c["exchange_ms"]  # the 857 MB all-gather bounds this layout


def test_gather_locality_clamps_the_ceiling():
    """products-local runs faster than the uniform-gather bound (L2 hits): the ceiling is the
    measured time and the note says why, so ceiling.frac == frac rather than below it."""
    rl = _check(bench.roofline(n=N, rows=N, nnz=NNZ, F_local=F, esz=4, avg_iter_ms=4.0, fs=F,
                               r=0, lpe=1), 4.0)
    assert rl["ceiling"]["clamped_to_measured"]
    assert rl["ceiling"]["frac"] == pytest.approx(rl["frac"])
    assert "locality" in rl["note"]


def test_kernel_plan_names_what_runs():
    sb = {"width": 4, "entries": 10, "value_free": True, "row_passes": 1, "launches": 0}
    desc, key, fs, r, lpe = bench.kernel_plan(100, 10, 4, sb)
    assert (fs, r, lpe) == (96, 4, 1) and key == "k_step[0,96)+k_rem_persist<W4,vf>[96,100)"
    assert bench.kernel_plan(100, 10, 0, None)[1] == "k_step"
    sb16 = dict(sb, width=16, value_free=False, row_passes=4)
    desc, key, fs, r, lpe = bench.kernel_plan(13, 10, 13, sb16)
    assert (fs, r, lpe) == (0, 13, 4) and key == "k_rem_persist<W16>[0,13)"
    # K = 1 never splits
    assert bench.kernel_plan(100, 1, 4, sb)[1] == "k_step"


def test_traffic_key_tracks_kernels_and_sources():
    k1 = bench.traffic_key("products-synth", "f32", "k_step", 100, N)
    k2 = bench.traffic_key("products-synth", "f32", "k_step[0,96)+k_rem_persist<W4>", 100, N)
    k3 = bench.traffic_key("products-synth", "f32", "k_step", 100, N // 8 + 1, overlap=True)
    assert len({k1, k2, k3}) == 3
    assert k1.startswith(f"products-synth:f32:k_step:F100:rows{N}:src=")
    assert ":ov:" in k3
    assert bench.committed_traffic("no-such-key") is None


def test_cpu_leg_threads_and_sample(monkeypatch):
    """N > 1: torch.distributed.run sets OMP_NUM_THREADS=1 per rank, but rank 0 runs the CPU leg
    while the others wait, so it takes up to 16 visible CPUs; N = 1 keeps the box's share.  The
    leg runs all K iterations at every N (its Z_K is every line's parity reference)."""
    monkeypatch.setattr(bench.os, "sched_getaffinity", lambda pid: set(range(64)), raising=False)
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert bench.cpu_threads(1) == (1, 64)
    assert bench.cpu_threads(8) == (16, 64)
    monkeypatch.setenv("OMP_NUM_THREADS", "32")
    assert bench.cpu_threads(8) == (32, 64)
    monkeypatch.setattr(bench.os, "sched_getaffinity", lambda pid: set(range(4)), raising=False)
    assert bench.cpu_threads(8) == (4, 4)
    assert bench.parse([]).cpu_iters is None  # None: all K iterations, N = 1 and N > 1
    assert not hasattr(bench, "CPU_LEG_WORK")


class _StubGraph:
    """What bench reads from a rank's graph: its held rows and nnz (no HIP library)."""

    def __init__(self, n, lo, hi):
        self.n, self.rows, self.nnz_hat = n, hi - lo, 10 * (hi - lo)

    def shard_offsets(self, nshards, shard_rows):  # the pipelined row steps' shard ranges
        pass


def _noop_step(runner, src, out_rows, k, part):
    pass


def _key_worker(rank, world, init, q):
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        from ppnp_amd.dist import Layout, NullComm, PartitionedAPPNP, relayed

        n, f = 1000, 100
        H = torch.zeros(n, f)
        out = []
        cases = [("col", False, "group"), ("row", True, "group"), ("row", False, "group")]
        if world == 4:
            cases.append(("2x2", True, "group"))
        if world == 6:  # R >= 3 row groups x 2 column groups: pipelined unless relayed
            cases += [("3x2", True, "group"), ("3x2", True, "multipath")]
        for spec, overlap, exchange in cases:
            layout = Layout.parse(spec, world)
            kw = dict(layout=layout, overlap=overlap, exchange=exchange,
                      graph_fn=lambda lo, hi, ov: _StubGraph(n, lo, hi), step_fn=_noop_step)
            real = PartitionedAPPNP.create(None, None, n, H, 10, 0.1, "cpu", **kw)
            # what bench.py --emulate builds for this candidate
            emu = PartitionedAPPNP.create(
                None, None, n, H, 10, 0.1, "cpu", rank=rank, world=world,
                comm=NullComm(broadcast=not relayed(layout, exchange)), **kw)
            out.append((spec, overlap, bench.rank_traffic_key("products-synth", "f32", real, 10),
                        bench.rank_traffic_key("products-synth", "f32", emu, 10)))
            out[-1] += (real.pipeline, emu.pipeline, exchange)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 6])
def test_emulated_rank_key_equals_real_rank_key(world):
    """VERDICT r3 missing #3: the traffic key names what a rank runs, not the layout's name, so
    rank r of a real P-rank run (a gloo process group here) and its single-GPU emulation
    (rank=r, world=P, NullComm: what --emulate P:r builds) look up the same committed PMC
    entry."""
    import tempfile
    import uuid

    import torch.multiprocessing as mp

    # file:// rendezvous: no port race; a directory of this user's own
    d = os.path.join(tempfile.gettempdir(), f"ppnp_rdv_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    init = "file://" + os.path.join(d, uuid.uuid4().hex)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    mp.start_processes(_key_worker, args=(world, init, q), nprocs=world, join=True,
                       start_method="spawn")
    res = dict(q.get() for _ in range(world))
    for r, rows in res.items():
        for spec, overlap, real, emu, real_pipe, emu_pipe, exchange in rows:
            assert real == emu, (r, spec, real, emu)
            assert "EMULATED" not in emu and "rows" in emu
            assert (":ov" in real) == (overlap and spec != "col")
            # the pipelined exchange from 3 row groups on, never on the relayed exchange
            rows_ = int(spec.split("x")[0]) if "x" in spec else (world if spec == "row" else 1)
            want = overlap and rows_ >= 3 and exchange != "multipath"
            assert real_pipe == emu_pipe == want, (r, spec, exchange, real_pipe, emu_pipe)
            assert (":pipe" in real) == want


def test_device_info_never_raises():
    """The bench line's ``device`` block is a diagnostic: without a GPU it reports the error
    instead of raising (on the box: name, PCI address, HBM vendor, clocks from sysfs)."""
    import torch

    info = bench.device_info(torch.device("cuda", 0))
    assert isinstance(info, dict)
    if not torch.cuda.is_available():
        assert "error" in info
    else:
        assert {"name", "pci", "vram_vendor", "mclk"} <= set(info)


def test_kernel_split_summarises_launches(monkeypatch):
    """roofline.kernel_ms from the per-launch list (ppnp_amd.ops.kernel_times stubbed: no GPU):
    per-kind mean / min / max, the per-iteration sum beside the timed iteration, and the
    per-launch list; an empty list (a captured plan records no launches) stays well-formed."""
    import torch

    import ppnp_amd.ops as ops

    seq = [("copy", 0.4)] + [("step", 7.4), ("rem", 0.77)] * 10
    monkeypatch.setattr(ops, "kernel_times", lambda fn, device: seq)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    k = bench.kernel_split(lambda: None, "cuda:0", 10, 8.2)
    assert k["main"]["launches"] == 10 and k["main"]["mean"] == pytest.approx(7.4)
    assert k["rem"]["mean"] == pytest.approx(0.77) and k["copy"]["launches"] == 1
    assert k["sum_of_kernels"] == pytest.approx((0.4 + 10 * (7.4 + 0.77)) / 10)
    assert k["iteration"] == 8.2 and len(k["ms_per_launch"]) == 21
    monkeypatch.setattr(ops, "kernel_times", lambda fn, device: [])
    k = bench.kernel_split(lambda: None, "cuda:0", 10, 8.2)
    # nothing recorded (a replayed plan) says so instead of empty stats
    assert "main" not in k and "no launches recorded" in k["note"] and k["iteration"] == 8.2
    # a row-partitioned rank: local / remote halves count as the SpMM kernel, the library's
    # exchange calls are listed but never counted as kernel time
    seq = [("copy", 0.3)] + [("local", 0.2), ("remote", 0.8), ("rem", 0.1), ("xchg", 1.5)] * 2
    monkeypatch.setattr(ops, "kernel_times", lambda fn, device: seq)
    k = bench.kernel_split(lambda: None, "cuda:0", 2, 2.0)
    assert k["main"]["launches"] == 4 and k["local"]["mean"] == pytest.approx(0.2)
    assert k["remote"]["mean"] == pytest.approx(0.8) and k["xchg"]["launches"] == 2
    assert k["sum_of_kernels"] == pytest.approx((0.3 + 2 * 1.1) / 2)


def test_plain_run_options_and_output_sample(tmp_path):
    """--full and --dump-outputs are off by default.  The dumped sample: every row of a block
    that fits, otherwise the same ascending, duplicate-free rows on every call, sized so that
    all ranks together stay within DUMP_MAX_BYTES as float32; the written file is float32."""
    import numpy as np
    import torch

    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    assert bench.DUMP_MAX_BYTES <= 64_000_000
    assert bench.dump_rows(1000, 100, 1) is None
    for rows, width, world in ((N, 100, 1), (N, 13, 8), (N // 8 + 1, 100, 8)):
        r = bench.dump_rows(rows, width, world)
        assert np.array_equal(r, bench.dump_rows(rows, width, world))
        assert r.min() >= 0 and r.max() < rows and np.all(np.diff(r) > 0)
        row = width * 4 * world  # float32 bytes of one sampled row over all ranks
        assert (len(r) + 1) * row > bench.DUMP_MAX_BYTES >= len(r) * row
    Z = torch.arange(12, dtype=torch.bfloat16).reshape(4, 3)
    bench.write_output(str(tmp_path / "out"), "Z", bench.sample_output(Z, 1))
    got = np.load(tmp_path / "out" / "Z.npy")
    assert got.dtype == np.float32 and np.array_equal(got, Z.float().numpy())
