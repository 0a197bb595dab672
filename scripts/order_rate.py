"""Cost of the opt-in per-item emitter count (baz_music_set_order_mode) at config 2's and config 3's shapes: mode 0, MDL and
AIC on one device in one session, alternating, device-resident batches, hip events (torch.cuda.Event) around `--steps`
back-to-back calls; and mode 0 of the PARENT commit's library in the same session, so that "mode 0 costs what it cost
before the mode existed" is a statement about one box at one time.

    python scripts/order_rate.py [--rounds 5] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/order_mode.txt]

--parent-lib: a libbaz_music_hip.so built from the parent commit (a git worktree of it + `python -m gr_baz_amd.build`).
Every (library, round) runs in a fresh child process (this file with --worker), one at a time.  Per leg and wiring (spectrum
port wired / not) the report gives the median and the spread of the per-round times, the MDL / AIC cost over mode 0, and --
from a separate pass with the library's per-stage events on -- the EVD stage alone: at config 3's shape (m = 8, n = 2) mode 0
finds the signal subspace by orthogonal iteration and the mode sends every item through the Jacobi, which is the share of the
cost that a count from the signal eigenvalues alone would win back.  Needs a gfx950 device (no fallback)."""
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
    # name, m, n (= n_max with the mode on), nsamples, res, batch
    ("cfg2", 4, 2, 1024, 3600, 16384),
    ("cfg3", 8, 2, 4096, 36000, 1024),
]
MODES = {"off": 0, "mdl": 1, "aic": 2}
STAGES = ("cov", "evd", "scan", "merge")


def worker(a):
    """One library, every leg and wiring, the modes it knows in alternation: one JSON line on stdout."""
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
    has_mode = hasattr(L, "baz_music_set_order_mode")
    if has_mode:
        L.baz_music_set_order_mode.argtypes = [vp, ctypes.c_int]
    modes = [m for m in a.modes.split(",") if m == "off" or has_mode]
    dev = torch.device("cuda:0")
    out = {"lib": a.lib, "has_mode": has_mode, "times_ms": {}, "evd_ms": {}}
    for name, m, n, N, res, B in LEGS:
        arr = synth.array_geometry(m)
        table = np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5, 1.0) for b in range(res)], dtype=np.complex64))
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        h = vp()
        r = L.baz_music_create(ctypes.byref(h), m, n, N, res, table.view(np.float32).ctypes.data_as(f32p), 0)
        if r != 0:
            raise SystemExit("baz_music_create: %d" % r)
        stream = vp(torch.cuda.current_stream().cuda_stream)

        def call(with_spec):
            rc = L.baz_music_process_device_on(h, stream, vp(x.data_ptr()), B, vp(ang.data_ptr()), vp(lvl.data_ptr()),
                                               vp(spec.data_ptr()) if with_spec else None)
            if rc != 0:
                raise SystemExit("baz_music_process_device_on: %d" % rc)

        L.baz_music_reserve(h, B)
        for wiring in ("spec", "nospec"):
            for rep in range(a.reps):                       # the modes alternate: off, mdl, aic, off, mdl, aic, ...
                for mode in modes:
                    if has_mode and L.baz_music_set_order_mode(h, MODES[mode]) != 0:
                        raise SystemExit("baz_music_set_order_mode")
                    for _ in range(a.warmup):
                        call(wiring == "spec")
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        call(wiring == "spec")
                    e1.record()
                    torch.cuda.synchronize()
                    out["times_ms"].setdefault("%s/%s/%s" % (name, wiring, mode), []).append(e0.elapsed_time(e1) / a.steps)
            for mode in modes:                              # the EVD stage alone, from the library's own events (a pass of its own)
                if has_mode:
                    L.baz_music_set_order_mode(h, MODES[mode])
                call(wiring == "spec")
                torch.cuda.synchronize()
                L.baz_music_profile(h, 1)
                for _ in range(a.steps):
                    call(wiring == "spec")
                torch.cuda.synchronize()
                st = {}
                for s, sname in enumerate(STAGES):
                    ms, cnt = ctypes.c_double(0.0), ctypes.c_uint64(0)
                    L.baz_music_stage_ms(h, s, ctypes.byref(ms), ctypes.byref(cnt))
                    st[sname] = ms.value / a.steps
                L.baz_music_profile(h, 0)
                out["evd_ms"]["%s/%s/%s" % (name, wiring, mode)] = st
        L.baz_music_destroy(h)
    print("ORDER_RATE " + json.dumps(out), flush=True)


def run_worker(lib, modes, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--modes", modes, "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--reps", "1"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith("ORDER_RATE ")][-1]
    return json.loads(line[len("ORDER_RATE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--own-modes", default="off,mdl,aic", help="modes timed on this tree's library (off alone: a plain A/B against the parent)")
    ap.add_argument("--parent-first", action="store_true", help="time the parent's library first in every round")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=OWN_LIB)
    ap.add_argument("--modes", default="off,mdl,aic")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    own, parent, stages = {}, {}, {}
    for _ in range(a.rounds):                               # own library and the parent's in alternation
        for which in (("parent", "own") if a.parent_first else ("own", "parent")):
            if which == "own":
                w = run_worker(OWN_LIB, a.own_modes, a)
                for k, v in w["times_ms"].items():
                    own.setdefault(k, []).extend(v)
                stages = w["evd_ms"]
            elif a.parent_lib:
                w = run_worker(a.parent_lib, "off", a)
                for k, v in w["times_ms"].items():
                    parent.setdefault(k, []).extend(v)
    lines = ["Opt-in per-item emitter count (baz_music_set_order_mode, DESIGN.md 8c): cost on one MI355X, one session",
             "scripts/order_rate.py --rounds %d --steps %d --warmup %d%s" % (a.rounds, a.steps, a.warmup, " --parent-lib <parent commit's library>" if a.parent_lib else ""),
             "ms per process_device call, device-resident batch, median [min .. max] over the rounds (a fresh process per round and library, alternating)", ""]
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))
    for name, m, n, N, res, B in LEGS:
        for wiring in ("spec", "nospec"):
            key = "%s/%s/" % (name, wiring)
            off = own[key + "off"]
            lines.append("%s  m=%d n=%d nsamples=%d res=%d batch=%d  spectrum port %s" % (name, m, n, N, res, B, "wired" if wiring == "spec" else "not wired"))
            if parent:
                p = parent[key + "off"]
                inside = min(p) <= statistics.median(off) <= max(p)
                lines.append("  parent commit, mode 0   %s" % fmt(p))
                lines.append("  this tree,     mode 0   %s   median %s the parent's spread" % (fmt(off), "inside" if inside else "OUTSIDE"))
            else:
                lines.append("  this tree,     mode 0   %s" % fmt(off))
            for mode in ("mdl", "aic"):
                if key + mode not in own:
                    continue
                v = own[key + mode]
                lines.append("  this tree,     %s      %s   x%.3f of mode 0" % (mode.upper(), fmt(v), statistics.median(v) / statistics.median(off)))
            s0, s1 = stages[key + "off"], stages.get(key + "mdl", stages[key + "off"])
            lines.append("  stages (library events, last round), mode 0 -> MDL:  " +
                         "  ".join("%s %.4f -> %.4f" % (sn, s0[sn], s1[sn]) for sn in STAGES))
            lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
