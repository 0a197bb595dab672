"""Cost and effect of the opt-in sub-bin angle refinement (baz_music_set_refine_mode) on one device in one session, the
variants alternating, device-resident batches, hip events (torch.cuda.Event) around `--steps` back-to-back calls:

  (a) mode 0 of this tree against the PARENT commit's library at config 2's shape, with and without the spectrum port;
  (b) mode 1 against mode 0 at config 1's and config 2's shapes, default wiring and port wired, peak mode 0 and 1;
  (c) what the feature is for: config 1's 360-bin table with peak mode and refinement against a 3,600-bin table on the same
      items without it -- items/s and the RMS angle error of both (emitters at 40.3 / 121.7 degrees, 40 dB).

    python scripts/refine_rate.py [--rounds 5] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/refine_mode.txt]

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
]
TRUTH = (40.3, 121.7)
EFFECT_BATCH = 16384


def rms_error(ang, lvl):
    a = ang.astype(np.float64)[..., None]
    e = (a - np.asarray(TRUTH) + 180.0) % 360.0 - 180.0
    e = np.take_along_axis(e, np.argmin(np.abs(e), axis=-1)[..., None], axis=-1)[..., 0]
    return float(np.sqrt(np.mean(e[lvl != 0] ** 2)))


def worker(a):
    """One library, every leg, wiring and variant it knows in alternation: one JSON line on stdout."""
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
    L.baz_music_set_peak_mode.argtypes = [vp, ctypes.c_int]
    has_mode = hasattr(L, "baz_music_set_refine_mode")
    if has_mode:
        L.baz_music_set_refine_mode.argtypes = [vp, ctypes.c_int]
    dev = torch.device("cuda:0")
    out = {"lib": a.lib, "has_mode": has_mode, "times_ms": {}, "effect": {}}

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
        variants = [(p, r) for p in (0, 1) for r in ((0, 1) if has_mode else (0,))] if has_mode else [(0, 0)]
        for wiring in ("spec", "nospec"):
            for peak, refine in variants:                              # the variants alternate inside a round
                if L.baz_music_set_peak_mode(h, peak) != 0 or (has_mode and L.baz_music_set_refine_mode(h, refine) != 0):
                    raise SystemExit("set mode")
                if has_mode and refine:
                    L.baz_music_reserve(h, B)
                t = timed(lambda: call(wiring == "spec"))
                out["times_ms"].setdefault("%s/%s/peak%d/refine%d" % (name, wiring, peak, refine), []).append(t)
        L.baz_music_destroy(h)

    if has_mode:                                                       # (c) coarse table + refinement against a fine table
        m, n, N, B = 4, 2, 256, EFFECT_BATCH
        arr, _ = table_of(m, 360)
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=40.0, seed=7, angles_deg=TRUTH)
        for label, res, peak, refine in (("360 bins, grid", 360, 1, 0), ("360 bins, refined", 360, 1, 1), ("3600 bins, grid", 3600, 1, 0),
                                         ("3600 bins, grid, reference top-n", 3600, 0, 0)):
            _, table = table_of(m, res)
            ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
            lvl = torch.zeros_like(ang)
            h = vp()
            if L.baz_music_create(ctypes.byref(h), m, n, N, res, table.view(np.float32).ctypes.data_as(f32p), 0) != 0:
                raise SystemExit("baz_music_create")
            L.baz_music_set_peak_mode(h, peak)
            L.baz_music_set_refine_mode(h, refine)
            L.baz_music_reserve(h, B)

            def call():
                if L.baz_music_process_device_on(h, stream, vp(x.data_ptr()), B, vp(ang.data_ptr()), vp(lvl.data_ptr()), None) != 0:
                    raise SystemExit("baz_music_process_device_on")

            t = timed(call)
            torch.cuda.synchronize()
            out["effect"][label] = {"ms": t, "items_per_s": B / (t * 1e-3), "rms_deg": rms_error(ang.cpu().numpy(), lvl.cpu().numpy())}
            L.baz_music_destroy(h)
    print("REFINE_RATE " + json.dumps(out), flush=True)


def run_worker(lib, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith("REFINE_RATE ")][-1]
    return json.loads(line[len("REFINE_RATE "):])


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
    own, parent, effect = {}, {}, {}
    for rnd in range(a.rounds):                               # own library and the parent's in alternation, the order alternating too
        for which in (("own", "parent") if rnd % 2 == 0 else ("parent", "own")):
            if which == "own":
                w = run_worker(OWN_LIB, a)
                for k, v in w["times_ms"].items():
                    own.setdefault(k, []).extend(v)
                for k, v in w["effect"].items():
                    effect.setdefault(k, []).append(v)
            elif a.parent_lib:
                w = run_worker(a.parent_lib, a)
                for k, v in w["times_ms"].items():
                    parent.setdefault(k, []).extend(v)
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))
    lines = ["Opt-in sub-bin angle refinement (baz_music_set_refine_mode, DESIGN.md 8d): cost and effect on one MI355X, one session",
             "scripts/refine_rate.py --rounds %d --steps %d --warmup %d%s" % (a.rounds, a.steps, a.warmup, " --parent-lib <parent commit's library>" if a.parent_lib else ""),
             "ms per process_device call, device-resident batch, median [min .. max] over the rounds (a fresh process per round and library, alternating)", ""]
    lines.append("(a) mode 0 against the parent commit's library, cfg2's shape")
    for wiring in ("spec", "nospec"):
        key = "cfg2/%s/peak0/refine0" % wiring
        off = own[key]
        lines.append("  spectrum port %s" % ("wired" if wiring == "spec" else "not wired"))
        if parent:
            p = parent[key]
            lines.append("    parent commit          %s" % fmt(p))
            lines.append("    this tree, mode 0      %s   median %s the parent's spread, ratio of medians %.4f"
                         % (fmt(off), "inside" if min(p) <= statistics.median(off) <= max(p) else "OUTSIDE", statistics.median(off) / statistics.median(p)))
        else:
            lines.append("    this tree, mode 0      %s" % fmt(off))
    lines += ["", "(b) mode 1 against mode 0"]
    for name, m, n, N, res, B in LEGS:
        for wiring in ("nospec", "spec"):
            lines.append("  %s  m=%d n=%d nsamples=%d res=%d batch=%d  spectrum port %s" % (name, m, n, N, res, B, "wired" if wiring == "spec" else "not wired (default wiring)"))
            for peak in (0, 1):
                v0 = own["%s/%s/peak%d/refine0" % (name, wiring, peak)]
                v1 = own["%s/%s/peak%d/refine1" % (name, wiring, peak)]
                lines.append("    peak mode %d   mode 0 %s   mode 1 %s   x%.3f  (+%.4f ms, %.2f ns per item)"
                             % (peak, fmt(v0), fmt(v1), statistics.median(v1) / statistics.median(v0), statistics.median(v1) - statistics.median(v0),
                                (statistics.median(v1) - statistics.median(v0)) * 1e6 / B))
    lines += ["", "(c) cfg1's items (m=4, 64 snapshots, 40 dB, emitters at %g / %g degrees, %d items), spectrum port not wired" % (TRUTH + (EFFECT_BATCH,))]
    for label, rows in effect.items():
        ms = [r["ms"] for r in rows]
        lines.append("  %-34s %s ms   %.3e items/s   RMS angle error %.4f deg" % (label, fmt(ms), EFFECT_BATCH / (statistics.median(ms) * 1e-3), rows[-1]["rms_deg"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
