"""Cost of the opt-in per-antenna calibration (baz_music_set_calibration / baz_music_calibrate_device) on one device in one session,
this tree's library and the PARENT commit's alternating, a fresh child process per (library, round):

  (a) wall time of baz_music_set_table (host clock around the call: it returns when the images are built and exchanged) at
      (4 antennas, 3,600 bins) and (8 antennas, 36,000 bins): the parent, this tree with the calibration off (launches the parent's
      kernels) and with it on (table_calib_kernel in place of the first copy_words_kernel launch); and of set_calibration itself;
  (b) the step time of the headline device-resident call (4 antennas, 1,024 samples, 3,600 bins, port wired, 16,384 items), hip events
      around `--steps` back-to-back calls: the parent against this tree with the calibration off;
  (c) baz_music_calibrate_device at 16,384 items of the headline shape: wall time of the call, split into the covariance stage
      (profiled under STAGE_COV), cov_mean_kernel's two launches (STAGE_MERGE) and the host eigen step (baz_music_calibration_estimate
      on the same R-bar, host clock).

    python scripts/calibration_rate.py [--rounds 3] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/calibration.txt]

Needs a gfx950 device (no fallback)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OWN_LIB = os.path.join(ROOT, "gr_baz_amd", "csrc", "libbaz_music_hip.so")

RETUNE_SHAPES = [("m4_3600bins", 4, 2, 1024, 3600), ("m8_36000bins", 8, 2, 4096, 36000)]
HEADLINE = (4, 2, 1024, 3600, 16384)
RETUNES = 60
STAGE_COV, STAGE_MERGE = 0, 3


def worker(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 device")
    from gr_baz_amd import synth
    L = ctypes.CDLL(a.lib)
    vp, u32, f32p, f64p = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    L.baz_music_create.argtypes = [ctypes.POINTER(vp), u32, u32, u32, u32, f32p, ctypes.c_int]
    L.baz_music_destroy.argtypes = [vp]
    L.baz_music_destroy.restype = None
    L.baz_music_reserve.argtypes = [vp, u32]
    L.baz_music_set_table.argtypes = [vp, f32p]
    L.baz_music_process_device_on.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.baz_music_profile.argtypes = [vp, ctypes.c_int]
    L.baz_music_stage_ms.argtypes = [vp, ctypes.c_int, f64p, ctypes.POINTER(ctypes.c_uint64)]
    has_mode = hasattr(L, "baz_music_set_calibration")
    if has_mode:
        L.baz_music_set_calibration.argtypes = [vp, f32p]
        L.baz_music_calibrate_device.argtypes = [vp, vp, u32, f32p, f64p, f64p, f64p]
        L.baz_music_calibration_estimate.argtypes = [u32, f64p, f32p, f64p, f64p]
    dev = torch.device("cuda:0")
    out = {"lib": a.lib, "has_mode": has_mode, "retune_ms": {}, "step_ms": {}, "calibrate_ms": {}}

    def table_of(m, res, scale=1.0):
        arr = synth.array_geometry(m)
        return arr, np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5, scale) for b in range(res)], dtype=np.complex64))

    def gains(m):
        rng = np.random.default_rng(5)
        return (rng.uniform(0.7, 1.3, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex64)

    def wall(call, reps):
        call()
        call()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    for name, m, n, N, res in RETUNE_SHAPES:
        _, t1 = table_of(m, res)
        _, t2 = table_of(m, res, 1.1)
        h = vp()
        if L.baz_music_create(ctypes.byref(h), m, n, N, res, t1.view(np.float32).ctypes.data_as(f32p), 0) != 0:
            raise SystemExit("baz_music_create")
        tabs = [t1.view(np.float32).ctypes.data_as(f32p), t2.view(np.float32).ctypes.data_as(f32p)]
        flip = [0]

        def retune():
            flip[0] ^= 1
            if L.baz_music_set_table(h, tabs[flip[0]]) != 0:
                raise SystemExit("baz_music_set_table")

        out["retune_ms"][name + "/off"] = wall(retune, RETUNES)
        if has_mode:
            g = [gains(m), np.conj(gains(m))]
            gp = [x.view(np.float32).ctypes.data_as(f32p) for x in g]
            if L.baz_music_set_calibration(h, gp[0]) != 0:
                raise SystemExit("baz_music_set_calibration")
            out["retune_ms"][name + "/on"] = wall(retune, RETUNES)

            def recal():
                flip[0] ^= 1
                if L.baz_music_set_calibration(h, gp[flip[0]]) != 0:
                    raise SystemExit("baz_music_set_calibration")

            out["retune_ms"][name + "/set_calibration"] = wall(recal, RETUNES)
            L.baz_music_set_calibration(h, None)
            out["retune_ms"][name + "/off_again"] = wall(retune, RETUNES)
        L.baz_music_destroy(h)

    m, n, N, res, B = HEADLINE
    arr, table = table_of(m, res)
    x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
    ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
    lvl = torch.zeros_like(ang)
    spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
    h = vp()
    if L.baz_music_create(ctypes.byref(h), m, n, N, res, table.view(np.float32).ctypes.data_as(f32p), 0) != 0:
        raise SystemExit("baz_music_create")
    L.baz_music_reserve(h, B)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def call():
        if L.baz_music_process_device_on(h, stream, vp(x.data_ptr()), B, vp(ang.data_ptr()), vp(lvl.data_ptr()), vp(spec.data_ptr())) != 0:
            raise SystemExit("baz_music_process_device_on")

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    out["step_ms"]["headline/off"] = e0.elapsed_time(e1) / a.steps

    if has_mode:
        ref = np.ones(m, np.complex64)
        g, q, rbar = np.zeros(2 * m), ctypes.c_double(0.0), np.zeros(2 * m * m)
        gp_, rp = g.ctypes.data_as(f64p), rbar.ctypes.data_as(f64p)
        refp = ref.view(np.float32).ctypes.data_as(f32p)

        def cal():
            if L.baz_music_calibrate_device(h, vp(x.data_ptr()), B, refp, gp_, ctypes.byref(q), rp) != 0:
                raise SystemExit("baz_music_calibrate_device")

        out["calibrate_ms"]["call"] = wall(cal, 20)
        L.baz_music_profile(h, 1)
        for _ in range(10):
            cal()
        for stage, key in ((STAGE_COV, "covariance"), (STAGE_MERGE, "cov_mean_kernel")):
            ms, cnt = ctypes.c_double(0.0), ctypes.c_uint64(0)
            L.baz_music_stage_ms(h, stage, ctypes.byref(ms), ctypes.byref(cnt))
            out["calibrate_ms"][key] = ms.value / 10
            out["calibrate_ms"][key + "_launches_per_call"] = cnt.value / 10
        L.baz_music_profile(h, 0)
        out["calibrate_ms"]["host_eigen"] = wall(lambda: L.baz_music_calibration_estimate(m, rp, refp, gp_, ctypes.byref(q)), 200)
        out["calibrate_ms"]["quality"] = q.value
    L.baz_music_destroy(h)
    print("CALIB_RATE " + json.dumps(out), flush=True)


def run_worker(lib, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    print("worker done: %s" % lib, flush=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("CALIB_RATE ")][-1]
    return json.loads(line[len("CALIB_RATE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=OWN_LIB)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    own, parent = {}, {}
    for rnd in range(a.rounds):                               # own library and the parent's in alternation, the order alternating too
        for which in (("own", "parent") if rnd % 2 == 0 else ("parent", "own")):
            if which == "parent" and not a.parent_lib:
                continue
            w = run_worker(OWN_LIB if which == "own" else a.parent_lib, a)
            into = own if which == "own" else parent
            for group in ("retune_ms", "step_ms", "calibrate_ms"):
                for k, v in w[group].items():
                    into.setdefault(group + "/" + k, []).append(v)
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))

    def against_parent(key):
        if not parent:
            return ""
        p, v = parent[key], own[key]
        return "   median %s the parent's spread, ratio of medians %.4f" % (
            "inside" if min(p) <= statistics.median(v) <= max(p) else "OUTSIDE", statistics.median(v) / statistics.median(p))

    lines = ["Opt-in per-antenna calibration (baz_music_set_calibration, DESIGN.md 8h): cost on one MI355X, one session",
             "scripts/calibration_rate.py --rounds %d --steps %d --warmup %d%s" % (a.rounds, a.steps, a.warmup, " --parent-lib <parent commit's library>" if a.parent_lib else ""),
             "median [min .. max] over the rounds (a fresh process per round and library, alternating)", "",
             "baz_music_set_table, wall ms per call (median of %d calls per round)" % RETUNES]
    for name, m, n, N, res in RETUNE_SHAPES:
        lines.append("%s  m=%d res=%d (%d KiB of table)" % (name, m, res, m * res * 8 // 1024))
        if parent:
            lines.append("  parent commit                       %s" % fmt(parent["retune_ms/%s/off" % name]))
        lines.append("  this tree, calibration off          %s%s" % (fmt(own["retune_ms/%s/off" % name]), against_parent("retune_ms/%s/off" % name)))
        lines.append("  this tree, on and off again         %s" % fmt(own["retune_ms/%s/off_again" % name]))
        lines.append("  this tree, calibration on           %s" % fmt(own["retune_ms/%s/on" % name]))
        lines.append("  baz_music_set_calibration itself    %s" % fmt(own["retune_ms/%s/set_calibration" % name]))
    m, n, N, res, B = HEADLINE
    lines += ["", "headline device-resident call  m=%d n=%d nsamples=%d res=%d batch=%d, port wired; ms per call" % (m, n, N, res, B)]
    if parent:
        lines.append("  parent commit                       %s" % fmt(parent["step_ms/headline/off"]))
    lines.append("  this tree, calibration off          %s%s" % (fmt(own["step_ms/headline/off"]), against_parent("step_ms/headline/off")))
    lines += ["", "baz_music_calibrate_device, %d items of the headline shape; ms per call" % B,
              "  the call (host clock)               %s" % fmt(own["calibrate_ms/call"]),
              "  covariance stage (STAGE_COV)        %s   %g launches per call" % (fmt(own["calibrate_ms/covariance"]), own["calibrate_ms/covariance_launches_per_call"][0]),
              "  cov_mean_kernel (STAGE_MERGE)       %s   %g launches per call" % (fmt(own["calibrate_ms/cov_mean_kernel"]), own["calibrate_ms/cov_mean_kernel_launches_per_call"][0]),
              "  host eigen step                     %s" % fmt(own["calibrate_ms/host_eigen"]), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
