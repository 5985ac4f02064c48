"""GPU: the bench.py contract the driver depends on -- one JSON line on stdout with the metric.
A plain run times exactly the steps asked for and can dump the outputs of its last step; with
--full the line also carries the roofline and cpu_baseline objects.  Covered: the plain run and
its --dump-outputs files; the small workload at N=1 with --full; the driver's EXACT command line
(default workload C4, --steps 20 --warmup 5) with --full under a small wall budget; the
`python bench.py --gpus 2` form, which starts its own ranks (two bond-sharded ranks sharing the
test GPU, gloo-staged collectives); and the same two ranks started by a launcher."""

import json
import os
import socket
import subprocess
import sys
import time

import pytest

from helpers.ranks import run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config")
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline")


class _Done:
    def __init__(self, returncode, stdout, stderr):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr


def _run_bench(cmd, timeout, env=None):
    """subprocess.run(capture_output=True) with the child's progress notes (stderr) ALSO appended to
    gpurun_out/bench_contract_progress.txt as they come: a run of several minutes under captured output looks hung to a
    watchdog that only sees stdout, stderr and that directory."""
    import threading

    prog_dir = os.path.join(ROOT, "gpurun_out")
    os.makedirs(prog_dir, exist_ok=True)
    err = []
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env)

    def pump():
        with open(os.path.join(prog_dir, "bench_contract_progress.txt"), "a") as f:
            for line in p.stderr:
                err.append(line)
                f.write(line)
                f.flush()

    th = threading.Thread(target=pump, daemon=True)
    th.start()
    killer = threading.Timer(timeout, p.kill)  # stdout is one line: read to the end of the run, bounded by the timer
    killer.start()
    try:
        out = p.stdout.read()
        p.wait()
    finally:
        killer.cancel()
    th.join(10)
    return _Done(p.returncode, out, "".join(err))


def _line(out):
    # stdout carries the JSON line and NOTHING else (library banners -- gloo, RCCL -- are sent to stderr)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out
    return json.loads(lines[0])


def _check_plain(o):
    """what every line carries, a plain run's included"""
    for k in PLAIN_KEYS:
        assert k in o, k
    assert o["metric"] == "tdvp_sweeps_per_sec" and o["unit"] == "sweeps/s"
    assert o["higher_is_better"] is True and o["vs_baseline"] is None and o["data"] == "synthetic" and o["dtype"] == "c128"
    units = o["n_gpus"] if o["scaling"] == "weak" else 1  # replicas: every rank runs its own sweeps
    # a plain C4 run: a step is a piece of a half-sweep; the value counts the half-sweeps the timed pieces make up
    half_sweeps = o["config"].get("half_sweeps_timed", o["steps"])
    assert abs(o["value"] - units * half_sweeps * 1e3 / (o["steps"] * o["ms_per_step"])) < 1e-6 * o["value"]


def _check_common(o):
    _check_plain(o)
    for k in KEYS:
        assert k in o, k
    assert "workload" in o["config"] and "model" not in o["config"]
    r = o["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert 0 < r["frac"] <= 1.0, r  # a utilisation: executed work over the peak, never above 1
    assert 1 <= o["steps"] <= o["steps_requested"] and 1 <= o["warmup"]


def _check_secondary(rec, name):
    """one short leg of another BASELINE config under the `secondary` key: value, ms_per_step, roofline, cpu_baseline"""
    assert "error" not in rec, rec
    assert rec["workload"].startswith(name) and rec["unit"] == "sweeps/s" and rec["steps"] >= 2
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]
    r = rec["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] <= 1.0
    assert "traffic_source" in r
    c = rec["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["unit"] == "sweeps/s" and c["sample"] and "cpu_model" in c
    assert c["pinned"] is True and c["socket"] is not None and c["cores"] >= 1  # one socket, its physical cores
    cfg = rec["config"]
    if cfg["integrator"] == "lanczos":  # unitary: the norm stays 1 and the energy where it was
        assert abs(cfg["norm_after"] - 1) < 1e-10
        assert abs(cfg["energy_after"] - cfg["energy_before"]) < 1e-7 * max(1.0, abs(cfg["energy_before"]))
    b = rec["breakdown_ms"]
    assert b["wall"] > 0 and b["launches"] > 0


def _run_plain(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "C2", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return _line(p.stdout)


def test_bench_plain_run_times_the_steps_asked_for_and_dumps_its_outputs(tmp_path):
    """A plain run: exactly --steps timed and --warmup warm-up steps, only the headline figures, and with --dump-outputs
    the state of the last timed step as float64 .npy files, the same from run to run (seeded inputs)."""
    import numpy as np

    o = _run_plain(tmp_path / "a", 7, 2)
    _check_plain(o)
    assert o["n_gpus"] == 1 and o["steps"] == 7 and o["warmup"] == 2
    assert o["config"]["workload"].startswith("C2") and abs(o["config"]["norm_after"] - 1) < 1e-10
    for k in ("roofline", "breakdown_ms", "cpu_baseline", "secondary"):
        assert k not in o, k
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == ["energy.npy", "mps_sample.npy", "mps_sample_index.npy", "mps_shapes.npy", "norm.npy"], names
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(x.dtype == np.float64 for x in a.values()) and sum(x.nbytes for x in a.values()) <= 64 << 20
    L = 10
    assert a["mps_shapes"].shape == (L, 3) and a["mps_sample"].shape == a["mps_sample_index"].shape
    assert a["mps_sample"].shape[1] == 2 and np.isfinite(a["mps_sample"]).all() and np.abs(a["mps_sample"]).max() > 0
    assert sorted(set(a["mps_sample_index"][:, 0].astype(int))) == list(range(L))
    assert abs(a["norm"][0] - 1) < 1e-10 and np.isfinite(a["energy"]).all()
    b_line = _run_plain(tmp_path / "b", 7, 2)
    assert b_line["steps"] == 7
    for n in names:
        b = np.load(tmp_path / "b" / n)
        assert b.shape == a[n[:-4]].shape and np.allclose(b, a[n[:-4]], rtol=1e-9, atol=1e-12), n


def test_bench_plain_c4_steps_are_pieces_of_a_half_sweep(tmp_path):
    """The default workload in a plain run: a step is one of 8 pieces of a C4 half-sweep (the library's sweep_part), so
    tens of steps fit minutes; the value is still sweeps/s, counted by the pieces' shares of a half-sweep."""
    import numpy as np

    import bench

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    o = _line(p.stdout)
    _check_plain(o)
    cfg = o["config"]
    assert cfg["workload"].startswith("C4") and cfg["steps_per_half_sweep"] == 8
    pieces = bench.half_sweep_pieces(64, 16, 1024, 32, 8)
    assert cfg["half_sweep_pieces"] == [n for n, _ in pieces] and sum(cfg["half_sweep_pieces"]) == 64
    assert cfg["half_sweeps_timed"] == pytest.approx(sum(s for _, s in pieces[1:4]), rel=1e-12)  # pieces 2-4 timed
    assert o["steps"] == 3 and o["warmup"] == 1 and abs(cfg["norm_after"] - 1) < 1e-10
    assert 1e3 < o["ms_per_step"] < 30e3, o["ms_per_step"]
    assert abs(np.load(tmp_path / "norm.npy")[0] - 1) < 1e-10 and np.isfinite(np.load(tmp_path / "energy.npy")).all()


@pytest.mark.parametrize("shape", [(10, 10, 32, 6), (6, 32, 128, 16), (6, 16, 256, 8)], ids=["C2", "C3", "D256"])
def test_sweep_in_pieces_is_the_library_sweep(shape):
    """Half-sweeps run in pieces (engine.sweep_part, what bench.py times on C4) do the same work and leave the same state,
    bit for bit, as whole half-sweeps (engine.sweep), bonds of 256 included (the identity short-cut of the bond
    exponentials); a whole half-sweep is refused while one in pieces is in progress."""
    import numpy as np

    import bench
    from pytdscf_amd import TDVPEngine
    from pytdscf_amd import synthetic as syn

    L, d, D, M = shape
    dt = 0.5
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    engs = []
    try:
        for _ in range(2):
            e = TDVPEngine(L, device=0)
            engs.append(e)
            e.set_mpo(mpo)
            e.init_random([d] * L, D, seed=1)
            e.counters_reset()
        ref, part = engs
        ps = bench.PieceSweeper(part, dt, bench.half_sweep_pieces(L, d, D, M, 3))
        for forward in (True, False, True):
            ref.sweep(dt, forward)
            for k in range(3):
                ps.step()
                if k == 0:
                    with pytest.raises(ValueError, match="in parts is in progress"):
                        part.sweep(dt, forward)
            for a, b in zip(ref.get_mps(), part.get_mps()):
                assert np.array_equal(a, b)
        cr, cp = ref.counters(), part.counters()
        work = [k for k in cr if k.startswith("n_") or k.endswith("_flops")]
        assert work and {k: cr[k] for k in work} == {k: cp[k] for k in work}
    finally:
        for e in engs:
            e.close()


def test_bench_single_gpu_contract():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "C2", "--steps", "4", "--warmup", "1",
                        "--full", "--secondary", "C3", "--secondary-seconds", "40"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    o = _line(p.stdout)
    _check_common(o)
    assert o["n_gpus"] == 1 and o["steps"] == 4 and o["warmup"] == 1
    c = o["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "sweeps/s" and c["sample"]
    assert "cpu_model" in c and c["pinned"] is True and c["affinity_cpus"] >= c["cores"] >= 1
    assert abs(o["config"]["norm_after"] - 1) < 1e-10
    # the C2 traffic figure comes from a pass of the one-launch kernel, the C3 one from a pass of the form that ran
    assert o["roofline"]["traffic_source"].endswith("c2_traffic.json")
    assert o["secondary"]["C3"]["roofline"]["apply_form"] in o["secondary"]["C3"]["roofline"]["traffic_source"]
    assert o["config"]["secondary_summary"]["C3"]["value"] == pytest.approx(o["secondary"]["C3"]["value"], rel=1e-4)
    # energy conservation of the run itself, on one GPU as well
    assert abs(o["config"]["energy_after"] - o["config"]["energy_before"]) < 1e-7 * max(1.0, abs(o["config"]["energy_before"]))
    assert list(o["secondary"]) == ["C3"]
    _check_secondary(o["secondary"]["C3"], "C3")


def test_bench_driver_command_line_fits_its_wall_budget():
    """`python3 bench.py --gpus 1 --steps 20 --warmup 5 --full` is the driver's command with everything the
    benchmark measures (600 s limit).  On the default workload (C4: about a minute per sweep) 25 sweeps do not fit:
    the --full run must cut them to the wall budget, say so, and still print the full line.  The budget is set low here
    (one warm-up + one timed sweep + the CPU sample) to keep the test short."""
    t0 = time.time()
    p = _run_bench([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"],
                   timeout=660, env=dict(os.environ, MITDVP_BENCH_BUDGET="150"))
    wall = time.time() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    o = _line(p.stdout)
    _check_common(o)
    assert o["config"]["workload"].startswith("C4") and o["config"]["D"] == 1024 and o["config"]["L"] == 64
    assert o["steps_requested"] == 20 and o["warmup_requested"] == 5 and o["steps"] < 20
    assert o["roofline"]["bound"] == "mfma" and o["roofline"]["unit"] == "TFLOP/s"
    assert o["roofline"]["algorithmic_tflops"] >= o["roofline"]["achieved"]
    assert o["cpu_baseline"]["value"] > 0
    assert abs(o["config"]["norm_after"] - 1) < 1e-10
    assert abs(o["config"]["energy_after"] - o["config"]["energy_before"]) < 1e-7 * max(1.0, abs(o["config"]["energy_before"]))
    assert o["roofline"]["traffic_source"] and o["roofline"]["traffic_source"].startswith("profiles/")
    # the dominant kernel by itself: the two large launches of the apply, executed flop over their own HIP-event time
    st = o["roofline"]["stage_executed_tflops"]
    assert len(st) == 3 and 0 < st[0] <= 78.6 and 0 < st[2] <= 78.6
    assert abs(o["roofline"]["dominant_kernel_frac"] - max(st[0], st[2]) / 78.6) < 1e-12
    assert o["roofline"]["dominant_kernel_frac"] >= o["roofline"]["frac"] - 1e-12  # the whole apply cannot beat its best stage
    # the other BASELINE configs ride on the same line, driver-observed
    assert sorted(o["secondary"]) == ["C2", "C3", "C5"]
    for w in ("C2", "C3", "C5"):
        _check_secondary(o["secondary"][w], w)
        assert o["config"]["secondary_summary"][w]["value"] == pytest.approx(o["secondary"][w]["value"], rel=1e-4)
        src = o["secondary"][w]["roofline"]["traffic_source"]
        assert src is None or w.lower() in src.lower() or "D%d_" % o["secondary"][w]["config"]["D"] in src, src
    # the driver keeps the parsed `config` and a tail of stdout: the summary rides in `config`, the line stays short
    assert len(json.dumps(o["secondary"])) < 8192 and len(p.stdout) < 14000, (len(json.dumps(o["secondary"])), len(p.stdout))
    assert wall < 520, wall  # budget 150 s + at most one sweep + the CPU sample + the secondary legs (100 s)


def test_bench_plain_multi_gpu_command_launches_its_own_ranks():
    """`python bench.py --gpus 2`: starts its own ranks; the default partitioning is by site ranges."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "C2", "--steps", "2", "--warmup", "2",
           "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    o = _line(p.stdout)
    _check_common(o)
    assert o["n_gpus"] == 2 and o["scaling"] == "strong", p.stderr[-3000:]
    assert "site ranges" in o["config"]["parallelism"] and o["config"]["halo_messages"] > 0
    assert abs(o["config"]["norm_after"] - 1) < 1e-3  # the site-sharded scheme keeps the norm to O(dt^2)


def test_bench_plain_multi_gpu_command_bond_sharded():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "C2", "--steps", "2", "--warmup", "1",
           "--full", "--parallel", "tp"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    o = _line(p.stdout)
    _check_common(o)
    assert o["n_gpus"] == 2 and o["scaling"] == "strong" and o["config"]["collectives"] > 0, p.stderr[-3000:]
    assert "bond-sharded" in o["config"]["parallelism"] and abs(o["config"]["norm_after"] - 1) < 1e-10


def test_bench_two_ranks_bond_sharded():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", MITDVP_DIST_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "C2", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--parallel", "tp"]
    rcs, outs = run_ranks([cmd] * 2, [dict(env, RANK=str(r), LOCAL_RANK="0") for r in range(2)], timeout=600, cwd=ROOT,
                          split_stderr=True)
    assert rcs == [0, 0], "\n".join(o[1][-1500:] for o in outs)
    o = _line(outs[0][0])
    assert not [l for l in outs[1][0].splitlines() if l.startswith("{")]  # only rank 0 prints
    assert o["n_gpus"] == 2 and o["scaling"] == "strong" and o["config"]["collectives"] > 0
    assert "bond-sharded" in o["config"]["parallelism"] and abs(o["config"]["norm_after"] - 1) < 1e-10
