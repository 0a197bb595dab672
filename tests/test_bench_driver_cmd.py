"""What is graded, run as graded: the driver's command line

    python bench.py --gpus 1 --steps 20 --warmup 5

must exit 0 and leave on stdout exactly ONE JSON object (the contract) with BASELINE.json's metric, timed over exactly the 20 steps, and
--dump-outputs must write what the last of them computed.  The same command with --full must also carry a `roofline` whose fraction lies
in (0, 1), a `cpu_baseline` with a positive value, the in-run verification green and no failed secondary leg.  Round 5's driver run died
with a GPU memory fault inside a secondary leg before anything had been printed; since round 6 the measuring process of --full hands its
complete line to a supervising parent (and to stderr) BEFORE the secondary legs start -- each of which runs in its own process -- and the
same line, enriched, after them; the parent prints the last one it has got.  The second half of this file makes a leg fail (an exception,
a leg that never returns) and the measuring process fail after its first line, and checks that a complete line comes out every time."""
import importlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = json.load(open(os.path.join(ROOT, "BASELINE.json")))
DRIVER_ARGV = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
FULL_ARGV = DRIVER_ARGV + ["--full"]


def _run(argv, env=None, timeout=900):
    e = dict(os.environ, **(env or {}))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py"] + argv, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=e)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return r, lines


def _early_line(r):
    """The complete line the measuring process put out before the legs (stderr copy)."""
    tag = "complete line before the legs: "
    got = [l.split(tag, 1)[1] for l in r.stderr.splitlines() if tag in l]
    assert len(got) == 1, "expected one early line on stderr, found %d" % len(got)
    return json.loads(got[0])


def _check_complete(line, steps=20, warmup=5):
    assert BASELINE["metric"].startswith(line["metric"]), line["metric"]          # "MUSIC-DoA snapshots/s (4 ant, 1024 samp, 3600 bins)"
    assert line["unit"] == "snapshots/s" and line["n_gpus"] == 1 and line["steps"] == steps and line["warmup"] == warmup
    assert line["higher_is_better"] is True and line["vs_baseline"] is None and line["dtype"] == "f64" and line["data"] == "synthetic"
    assert line["value"] > 1e7                                                    # north_star's floor; the measured rate is ~2.3e8
    assert abs(line["value"] - line["config"]["items_per_step_all_gpus"] / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert "cfg2" in line["config"]["workload"] and "model" not in line["config"]
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert 0.0 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["launches"] >= steps and rf["avg_launch_ms"] > 0
    cb = line["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("reference", "port") and cb["unit"] == "snapshots/s" and cb["sample"]
    c = line["config"]
    assert c["verified_ok"] is True and c["verified_items"] >= 256 and c["verified_max_rel_err"] <= 1e-5 and c["verified_bins_identical"]
    assert c["headline_attempt"] == 1


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_the_drivers_command_is_the_headline_only_and_dumps_its_outputs(gpu_device, tmp_path):
    """The plain command times exactly --steps steps once, prints the headline line and nothing of --full; --dump-outputs holds what
    the last timed step computed (float32, at most 64 MB), and a sample of it agrees with the CPU oracle on the same seeded inputs."""
    import numpy as np
    import torch
    from gr_baz_amd import synth
    from helpers import assert_doa_match, assert_spectrum_close
    from oracle import music_ref as mr
    out = tmp_path / "outputs"
    r, lines = _run(DRIVER_ARGV + ["--dump-outputs", str(out)])
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-3000:])
    assert len(lines) == 1 and len(r.stdout.strip().splitlines()) == 1, "stdout must hold ONE JSON line, got %d" % len(lines)
    line = lines[0]
    assert BASELINE["metric"].startswith(line["metric"]) and line["unit"] == "snapshots/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["full"] is False and line["steps"] == 20 and line["warmup"] == 5
    assert line["rounds"]["count"] == 1 and line["rounds"]["steps_each"] == 20
    assert line["ms_per_step"] == pytest.approx(line["rounds"]["timed_seconds_total"] / 20 * 1e3, rel=1e-9)
    assert abs(line["value"] - line["config"]["items_per_step_all_gpus"] / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["value"] > 1e7
    for k in ("roofline", "cpu_baseline", "kernel_sources_sha"):
        assert k not in line, k
    assert "extra" not in line["config"] and "verified_ok" not in line["config"]
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(files) == sorted(line["outputs_dumped"]["files"]) == ["ang.npy", "lvl.npy", "spectrum_sample.npy"]
    assert all(a.dtype == np.float32 for a in files.values()) and sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
    B = line["config"]["items_per_gpu_per_step"]
    ang, lvl, spec = files["ang.npy"], files["lvl.npy"], files["spectrum_sample.npy"]
    assert ang.shape == lvl.shape == (B, 2) and spec.shape == (1024, 3600)
    # the sampled rows as bench.py draws them; check items of two streams against the oracle on the inputs regenerated from their seeds
    bench = importlib.import_module("bench")
    rows = np.sort(np.random.default_rng([bench.DUMP_SEED, 0]).choice(B, 1024, replace=False))
    arr, table = bench.helper_table(np, synth, bench.M, bench.RES)
    per = bench.ITEMS_PER_STREAM
    for s in (0, 7):
        pick = [i for i, r in enumerate(rows) if r // per == s][:4]
        assert pick
        x = synth.synth_stream(torch, gpu_device, per, bench.M, bench.NSAMPLES, arr, bench.FREQUENCY, bench.SPACING, seed=1002 + s)
        local = torch.from_numpy(rows[pick] % per).to(gpu_device)
        items = x.reshape(per, -1).index_select(0, local).cpu().numpy().view(np.complex64)
        ao, lo, so = mr.work_batch(np.ascontiguousarray(items), table, bench.M, 2)
        assert_spectrum_close(spec[pick], so)
        assert_doa_match(ang[rows[pick]], lvl[rows[pick]], ao, lo, bench.RES, strength64=so.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_the_drivers_exact_command(gpu_device):
    r, lines = _run(FULL_ARGV)
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-3000:])
    assert len(lines) == 1 and len(r.stdout.strip().splitlines()) == 1, "stdout must hold ONE JSON line, got %d" % len(lines)
    first, last = _early_line(r), lines[0]
    assert first["config"]["headline_attempt"] == 1 and first["config"]["headline_previous_failure"] is None
    _check_complete(first)
    _check_complete(last)
    assert first["value"] == last["value"] and first["roofline"] == last["roofline"]
    assert first["config"]["extras_pending"] > 0 and "extra" not in first["config"]
    c = last["config"]
    assert c["extras_pending"] == 0 and c["extras_run"] == len(c["extra"]) >= 13
    failed = {k: v["error"] for k, v in c["extra"].items() if "error" in v}
    assert not failed and c["extras_failed"] == 0 and c["extras_failed_legs"] == "", failed
    assert c["extras_all_verified_ok"] is True
    for k in ("default_wiring_snapshots_per_s", "incoherent_snapshots_per_s", "cfg3_snapshots_per_s", "cfg5_chain_snapshots_per_s",
              "wide_m64_snapshots_per_s", "retune_ms", "host_fed_pinned_with_port2_items_per_s"):
        assert c[k] and c[k] > 0, k
    print("\ndriver command: value %.4g snapshots/s, %.3f ms/step, roofline.frac %.3f, cpu_baseline %.3g on %d cores (%s); %d legs, %.0f s of legs"
          % (last["value"], last["ms_per_step"], last["roofline"]["frac"], last["cpu_baseline"]["value"], last["cpu_baseline"]["cores"],
             last["cpu_baseline"]["kind"], c["extras_run"], sum(v.get("leg_wall_s", 0) for v in c["extra"].values())))


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["raise", "hang"])
def test_a_fault_in_a_leg_cannot_take_the_line(gpu_device, kind):
    """hang = a leg that never returns (cut off by its time limit); raise = a Python exception; both before the leg's process touches the
    GPU.  Every time: rc 0, both lines complete, the failed leg named, the legs after it still measured."""
    legs = "cfg2_without_spectrum_port,wide_m64_n2,cfg2_snr60"
    env = {"BAZ_BENCH_INJECT_FAULT": "%s:wide_m64_n2" % kind}
    if kind == "hang":
        env["BAZ_BENCH_LEG_TIMEOUT_S"] = "45"      # (also the limit of the two healthy legs: 3 - 6 s each once the interpreter start is warm)
    r, lines = _run(FULL_ARGV + ["--legs", legs], env=env)
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-3000:])
    assert len(lines) == 1
    _check_complete(_early_line(r))
    _check_complete(lines[0])
    c = lines[0]["config"]
    assert c["extras_run"] == 3 and c["extras_failed"] == 1 and c["extras_failed_legs"] == "wide_m64_n2"
    assert "error" in c["extra"]["wide_m64_n2"]
    if kind == "hang":
        assert "timed out" in c["extra"]["wide_m64_n2"]["error"]
    for ok_leg in ("cfg2_without_spectrum_port", "cfg2_snr60"):                    # the leg before and the leg AFTER the fault
        assert "error" not in c["extra"][ok_leg] and c["extra"][ok_leg]["snapshots_per_s"] > 1e7 and c["extra"][ok_leg]["verified_ok"]
    assert c["default_wiring_snapshots_per_s"] > 1e7 and c["snr60_snapshots_per_s"] > 1e7 and c["wide_m64_snapshots_per_s"] is None


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_a_failure_in_the_measuring_process_after_its_line_keeps_that_line(gpu_device):
    """`python bench.py --full` measures in a child of itself.  The child fails AFTER its complete line and before the legs' figures: that line
    is the one line of stdout, and the exit code tells.  A failed child is never started again."""
    r, lines = _run(FULL_ARGV + ["--legs", "cfg2_snr60"], env={"BAZ_BENCH_INJECT_FAULT": "raise:after_first_line"})
    assert r.returncode == 1 and len(lines) == 1, (r.returncode, len(lines))
    _check_complete(lines[0])
    assert lines[0]["config"]["extras_pending"] == 1 and "extra" not in lines[0]["config"] and lines[0] == _early_line(r)
    assert "leg cfg2_snr60" not in r.stderr


def test_leg_table_and_driver_flags_on_cpu():
    """No GPU: the leg names are unique and known to the child mode, --help works, and a run without a GPU fails loudly (no CPU path)."""
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    r = subprocess.run([sys.executable, "bench.py", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    assert len(set(bench.LEG_ORDER)) == len(bench.LEG_ORDER) >= 13
    assert set(bench.MUSIC_LEGS) <= set(bench.LEG_ORDER)
    for must in ("cfg2_retune_in_flight", "cfg3", "wide_m32_n2", "wide_m64_n2", "cfg5_chain", "cfg2_host_fed_gr37_model"):
        assert must in bench.LEG_ORDER
    import torch
    if not torch.cuda.is_available():
        for argv in (DRIVER_ARGV, FULL_ARGV):
            r = subprocess.run([sys.executable, "bench.py"] + argv, capture_output=True, text=True, cwd=ROOT, timeout=300)
            assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)
        r = subprocess.run([sys.executable, "bench.py", "--extra-leg", "cfg3"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)
