"""Cost of the opt-in covariance averaging across stream items (baz_music_set_averaging) on one device in one session, the
variants alternating, device-resident batches, hip events (torch.cuda.Event) around `--steps` back-to-back calls:

  (a) mode off of this tree against the PARENT commit's library at config 2's shape, with and without the spectrum port;
  (b) mode on at W = 4, 8, 64 against mode off at config 1's and config 2's shapes, 8 antennas (config 3's shape, 1,024 items) and
      32 antennas -- at config 2's shape this includes losing the fused covariance + EVD kernel;
  (c) the averaging stage alone (baz_music_debug_average: average_kernel + average_history_kernel) against a plain double2 copy of
      the same R bytes on the same device: achieved bytes/s, counting R read once and R-bar written once for both.

    python scripts/averaging_rate.py [--rounds 5] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/averaging_mode.txt]

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
    # name, m, n, nsamples, res, batch
    ("cfg1", 4, 2, 256, 360, 65536),
    ("cfg2", 4, 2, 1024, 3600, 16384),
    ("m8", 8, 2, 4096, 36000, 1024),
    ("m32", 32, 2, 2048, 3600, 1024),
]
WINDOWS = (1, 4, 8, 64)
STAGE = [("m=4 (E = 16)", 4, 1 << 20), ("m=32 (E = 1024)", 32, 1 << 14)]     # 256 MiB of R each: input + output do not fit the last-level cache


def worker(a):
    """One library, every leg, wiring and window it knows in alternation: one JSON line on stdout."""
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
    L.baz_music_sync.argtypes = [vp]
    L.baz_music_set_stream.argtypes = [vp, vp]
    L.baz_music_process_device_on.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    has_mode = hasattr(L, "baz_music_set_averaging")
    if has_mode:
        L.baz_music_set_averaging.argtypes = [vp, u32, ctypes.c_double]
        L.baz_music_debug_average.argtypes = [vp, vp, u32, vp]
    dev = torch.device("cuda:0")
    out = {"lib": a.lib, "has_mode": has_mode, "times_ms": {}, "stage_ms": {}}

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
    legs = LEGS if has_mode else [l for l in LEGS if l[0] == "cfg2"]          # the parent's library: leg (a) only
    for name, m, n, N, res, B in legs:
        arr, table = table_of(m, res)
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        h = vp()
        if L.baz_music_create(ctypes.byref(h), m, n, N, res, table.view(np.float32).ctypes.data_as(f32p), 0) != 0:
            raise SystemExit("baz_music_create")

        def call(with_spec):
            if L.baz_music_process_device_on(h, stream, vp(x.data_ptr()), B, vp(ang.data_ptr()), vp(lvl.data_ptr()),
                                             vp(spec.data_ptr()) if with_spec else None) != 0:
                raise SystemExit("baz_music_process_device_on")

        L.baz_music_reserve(h, B)
        for wiring in ("spec", "nospec"):
            for W in (WINDOWS if has_mode else (1,)):                  # the windows alternate inside a round
                if has_mode:
                    if L.baz_music_set_averaging(h, W, 1.0) != 0:
                        raise SystemExit("baz_music_set_averaging")
                    L.baz_music_reserve(h, B)
                t = timed(lambda: call(wiring == "spec"))
                out["times_ms"].setdefault("%s/%s/W%d" % (name, wiring, W), []).append(t)
        L.baz_music_destroy(h)
        del x, spec

    if has_mode:                                                       # (c) the averaging stage alone against a copy
        side = torch.cuda.Stream()                                     # (a created stream: set_stream cannot select the default one)
        with torch.cuda.stream(side):
            for label, m, B in STAGE:
                E = m * m
                _, table = table_of(m, 64)
                h = vp()
                if L.baz_music_create(ctypes.byref(h), m, 2, m * 8, 64, table.view(np.float32).ctypes.data_as(f32p), 0) != 0:
                    raise SystemExit("baz_music_create")
                if L.baz_music_set_stream(h, vp(side.cuda_stream)) != 0:
                    raise SystemExit("baz_music_set_stream")
                src = torch.randn(B, E, dtype=torch.complex128, device=dev)
                dst = torch.empty_like(src)
                nbytes = src.numel() * 16
                t = timed(lambda: dst.copy_(src))
                out["stage_ms"].setdefault("%s/copy" % label, []).append([t, nbytes])
                for W in WINDOWS[1:]:
                    if L.baz_music_set_averaging(h, W, 1.0) != 0:
                        raise SystemExit("baz_music_set_averaging")

                    def stage():
                        if L.baz_music_debug_average(h, vp(src.data_ptr()), B, vp(dst.data_ptr())) != 0:
                            raise SystemExit("baz_music_debug_average")

                    t = timed(stage)
                    out["stage_ms"].setdefault("%s/W%d" % (label, W), []).append([t, nbytes])
                L.baz_music_sync(h)
                L.baz_music_destroy(h)
                del src, dst
    print("AVERAGING_RATE " + json.dumps(out), flush=True)


def run_worker(lib, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith("AVERAGING_RATE ")][-1]
    return json.loads(line[len("AVERAGING_RATE "):])


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
    own, parent, stage = {}, {}, {}
    for rnd in range(a.rounds):                               # own library and the parent's in alternation, the order alternating too
        for which in (("own", "parent") if rnd % 2 == 0 else ("parent", "own")):
            if which == "own":
                w = run_worker(OWN_LIB, a)
                for k, v in w["times_ms"].items():
                    own.setdefault(k, []).extend(v)
                for k, v in w["stage_ms"].items():
                    stage.setdefault(k, []).extend(v)
            elif a.parent_lib:
                w = run_worker(a.parent_lib, a)
                for k, v in w["times_ms"].items():
                    parent.setdefault(k, []).extend(v)
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))
    lines = ["Opt-in covariance averaging across stream items (baz_music_set_averaging, DESIGN.md 8e): cost on one MI355X, one session",
             "scripts/averaging_rate.py --rounds %d --steps %d --warmup %d%s" % (a.rounds, a.steps, a.warmup, " --parent-lib <parent commit's library>" if a.parent_lib else ""),
             "ms per process_device call, device-resident batch, median [min .. max] over the rounds (a fresh process per round and library, alternating)", ""]
    lines.append("(a) mode off against the parent commit's library, cfg2's shape")
    for wiring in ("spec", "nospec"):
        off = own["cfg2/%s/W1" % wiring]
        lines.append("  spectrum port %s" % ("wired" if wiring == "spec" else "not wired"))
        if parent:
            p = parent["cfg2/%s/W1" % wiring]
            lines.append("    parent commit          %s" % fmt(p))
            lines.append("    this tree, mode off    %s   median %s the parent's spread, ratio of medians %.4f"
                         % (fmt(off), "inside" if min(p) <= statistics.median(off) <= max(p) else "OUTSIDE", statistics.median(off) / statistics.median(p)))
        else:
            lines.append("    this tree, mode off    %s" % fmt(off))
    lines += ["", "(b) mode on (boxcar) against mode off"]
    for name, m, n, N, res, B in LEGS:
        for wiring in ("nospec", "spec"):
            lines.append("  %s  m=%d n=%d nsamples=%d res=%d batch=%d  spectrum port %s" % (name, m, n, N, res, B, "wired" if wiring == "spec" else "not wired (default wiring)"))
            v0 = own["%s/%s/W1" % (name, wiring)]
            lines.append("    off      %s" % fmt(v0))
            for W in WINDOWS[1:]:
                v1 = own["%s/%s/W%d" % (name, wiring, W)]
                lines.append("    W = %-3d  %s   x%.3f  (%+.4f ms, %.2f ns per item)"
                             % (W, fmt(v1), statistics.median(v1) / statistics.median(v0), statistics.median(v1) - statistics.median(v0),
                                (statistics.median(v1) - statistics.median(v0)) * 1e6 / B))
    lines += ["", "(c) the averaging stage alone (debug_average: average_kernel + average_history_kernel) against a double2 copy of the same R",
              "    bytes/s counts R read once + R-bar written once (what the copy moves); the kernel's own re-reads of R are not counted"]
    for label, m, B in STAGE:
        rows = stage["%s/copy" % label]
        ms = [r[0] for r in rows]
        nbytes = rows[0][1]
        copy_rate = 2 * nbytes / (statistics.median(ms) * 1e-3)
        lines.append("  %s, %d items, %.1f MiB of R" % (label, B, nbytes / 2.0 ** 20))
        lines.append("    copy     %s ms   %.3e bytes/s" % (fmt(ms), copy_rate))
        for W in WINDOWS[1:]:
            ms = [r[0] for r in stage["%s/W%d" % (label, W)]]
            rate = 2 * nbytes / (statistics.median(ms) * 1e-3)
            lines.append("    W = %-3d  %s ms   %.3e bytes/s   %.2f of the copy" % (W, fmt(ms), rate, rate / copy_rate))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
