"""Cost of the opt-in per-emitter Capon power estimate (baz_music_set_power_mode) on one device in one session, the variants
alternating, device-resident batches, hip events (torch.cuda.Event) around `--steps` back-to-back calls:

  (a) mode 0 of this tree against the PARENT commit's library at every leg (mode 0 launches the parent's kernels);
  (b) modes 1 and 2 against mode 0: items/s, and the time of power_kernel itself per item (the merge stage's profiled time with
      the mode on minus the same with it off).

Legs: the headline configuration (4 antennas, 1,024 samples, 3,600 bins) with and without the spectrum port, config 3 (8 antennas,
36,000 bins), and 16 antennas with 3 emitters.

    python scripts/power_rate.py [--rounds 5] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/power_mode.txt]

--parent-lib: a libbaz_music_hip.so built from the parent commit.  Every (library, round) runs in a fresh child process (this
file with --worker), one at a time.  The report gives the median and the spread of the per-round times.  Needs a gfx950 device
(no fallback)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OWN_LIB = os.path.join(ROOT, "gr_baz_amd", "csrc", "libbaz_music_hip.so")

LEGS = [
    # name, m, n, nsamples, res, batch, wirings
    ("headline", 4, 2, 1024, 3600, 16384, ("spec", "nospec")),
    ("cfg3", 8, 2, 4096, 36000, 4096, ("nospec",)),
    ("m16_n3", 16, 3, 1024, 360, 16384, ("nospec",)),
]
STAGE_MERGE = 3


def worker(a):
    """One library, every leg, wiring and mode it knows in alternation: one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 device")
    from gr_baz_amd import synth
    L = ctypes.CDLL(a.lib)
    vp, u32, f32p = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)
    L.baz_music_create.argtypes = [ctypes.POINTER(vp), u32, u32, u32, u32, f32p, ctypes.c_int]
    L.baz_music_destroy.argtypes = [vp]
    L.baz_music_destroy.restype = None
    L.baz_music_reserve.argtypes = [vp, u32]
    L.baz_music_process_device_on.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.baz_music_profile.argtypes = [vp, ctypes.c_int]
    L.baz_music_stage_ms.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    has_mode = hasattr(L, "baz_music_set_power_mode")
    if has_mode:
        L.baz_music_set_power_mode.argtypes = [vp, ctypes.c_int]
    dev = torch.device("cuda:0")
    out = {"lib": a.lib, "has_mode": has_mode, "times_ms": {}, "kernel_ns_per_item": {}}

    def table_of(m, res):
        arr = synth.array_geometry(m)
        return arr, np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5, 1.0) for b in range(res)], dtype=np.complex64))

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    stream = vp(torch.cuda.current_stream().cuda_stream)
    for name, m, n, N, res, B, wirings in LEGS:
        arr, table = table_of(m, res)
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev) if "spec" in wirings else None
        h = vp()
        if L.baz_music_create(ctypes.byref(h), m, n, N, res, table.view(np.float32).ctypes.data_as(f32p), 0) != 0:
            raise SystemExit("baz_music_create")

        def call(with_spec):
            if L.baz_music_process_device_on(h, stream, vp(x.data_ptr()), B, vp(ang.data_ptr()), vp(lvl.data_ptr()),
                                             vp(spec.data_ptr()) if with_spec else None) != 0:
                raise SystemExit("baz_music_process_device_on")

        def merge_ms(mode):
            """Profiled time of the merge stage per call (the stage power_kernel counts under)."""
            if has_mode and L.baz_music_set_power_mode(h, mode) != 0:
                raise SystemExit("set mode")
            L.baz_music_profile(h, 1)
            for _ in range(a.steps):
                call(False)
            torch.cuda.synchronize()
            ms, cnt = ctypes.c_double(0.0), ctypes.c_uint64(0)
            L.baz_music_stage_ms(h, STAGE_MERGE, ctypes.byref(ms), ctypes.byref(cnt))
            L.baz_music_profile(h, 0)
            return ms.value / a.steps

        L.baz_music_reserve(h, B)
        for wiring in wirings:
            for mode in ((0, 1, 2) if has_mode else (0,)):           # the modes alternate inside a round
                if has_mode:
                    if L.baz_music_set_power_mode(h, mode) != 0:
                        raise SystemExit("set mode")
                    L.baz_music_reserve(h, B)
                t = timed(lambda: call(wiring == "spec"))
                out["times_ms"].setdefault("%s/%s/mode%d" % (name, wiring, mode), []).append(t)
        if has_mode:
            base = merge_ms(0)
            out["kernel_ns_per_item"][name] = (merge_ms(1) - base) * 1e6 / B
        L.baz_music_destroy(h)
    print("POWER_RATE " + json.dumps(out), flush=True)


def run_worker(lib, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    print("worker done: %s" % lib, flush=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("POWER_RATE ")][-1]
    return json.loads(line[len("POWER_RATE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=OWN_LIB)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    own, parent, kern = {}, {}, {}
    for rnd in range(a.rounds):                               # own library and the parent's in alternation, the order alternating too
        for which in (("own", "parent") if rnd % 2 == 0 else ("parent", "own")):
            if which == "own":
                w = run_worker(OWN_LIB, a)
                for k, v in w["times_ms"].items():
                    own.setdefault(k, []).extend(v)
                for k, v in w["kernel_ns_per_item"].items():
                    kern.setdefault(k, []).append(v)
            elif a.parent_lib:
                w = run_worker(a.parent_lib, a)
                for k, v in w["times_ms"].items():
                    parent.setdefault(k, []).extend(v)
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))
    lines = ["Opt-in per-emitter Capon power estimate (baz_music_set_power_mode, DESIGN.md 8f): cost on one MI355X, one session",
             "scripts/power_rate.py --rounds %d --steps %d --warmup %d%s" % (a.rounds, a.steps, a.warmup, " --parent-lib <parent commit's library>" if a.parent_lib else ""),
             "ms per process_device call, device-resident batch, median [min .. max] over the rounds (a fresh process per round and library, alternating)", ""]
    for name, m, n, N, res, B, wirings in LEGS:
        for wiring in wirings:
            lines.append("%s  m=%d n=%d nsamples=%d res=%d batch=%d  spectrum port %s" % (name, m, n, N, res, B, "wired" if wiring == "spec" else "not wired (default wiring)"))
            v0 = own["%s/%s/mode0" % (name, wiring)]
            if parent:
                p = parent["%s/%s/mode0" % (name, wiring)]
                lines.append("  parent commit        %s   %.4e items/s" % (fmt(p), B / (statistics.median(p) * 1e-3)))
                lines.append("  this tree, mode 0    %s   %.4e items/s   median %s the parent's spread, ratio of medians %.4f"
                             % (fmt(v0), B / (statistics.median(v0) * 1e-3), "inside" if min(p) <= statistics.median(v0) <= max(p) else "OUTSIDE",
                                statistics.median(v0) / statistics.median(p)))
            else:
                lines.append("  this tree, mode 0    %s   %.4e items/s" % (fmt(v0), B / (statistics.median(v0) * 1e-3)))
            for mode in (1, 2):
                v = own["%s/%s/mode%d" % (name, wiring, mode)]
                lines.append("  this tree, mode %d    %s   %.4e items/s   x%.4f of mode 0  (+%.4f ms, %.2f ns per item)"
                             % (mode, fmt(v), B / (statistics.median(v) * 1e-3), statistics.median(v) / statistics.median(v0),
                                statistics.median(v) - statistics.median(v0), (statistics.median(v) - statistics.median(v0)) * 1e6 / B))
        lines.append("  power_kernel alone (merge stage profiled, mode 1 minus mode 0): %.2f ns per item [%.2f .. %.2f]; R traffic it adds: %d B/item against %d B/item of input"
                     % (statistics.median(kern[name]), min(kern[name]), max(kern[name]), 16 * m * m, 8 * N))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
