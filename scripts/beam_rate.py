"""Cost of the opt-in MVDR beamformer output (baz_music_set_beam_mode) on one device in one session, the variants alternating,
device-resident batches, hip events (torch.cuda.Event) around `--steps` back-to-back calls:

  (a) mode 0 of this tree against the PARENT commit's library at every leg (mode 0 launches the parent's kernels);
  (b) mode 1 against mode 0: items/s, and the time of the two new kernels per call (the merge stage's profiled time with the mode
      on minus the same with it off);
  (c) how close the two kernels come to their bytes: beam_apply_kernel moves 8 nsamples + 8 n K bytes per item; a plain device copy
      (torch copy_) that moves the same number of bytes, half read and half written, is timed beside it in the same process.  The
      time of BOTH kernels is charged to those bytes, so the fraction is a lower bound for beam_apply_kernel alone.

Legs: the headline configuration (4 antennas, 1,024 samples, 3,600 bins) with and without the spectrum port, config 3 (8 antennas,
36,000 bins), 16 antennas with 3 emitters, and the headline shape at a batch that leaves the 256 MiB Infinity Cache (1 GiB of input).

    python scripts/beam_rate.py [--rounds 3] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/beam_mode.txt]

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
    ("headline_1GiB", 4, 2, 1024, 3600, 131072, ("nospec",)),
]
STAGE_MERGE = 3


def beam_bytes(m, n, N):
    return 8 * N + 8 * n * (N // m)


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
    has_mode = hasattr(L, "baz_music_set_beam_mode")
    if has_mode:
        L.baz_music_set_beam_mode.argtypes = [vp, ctypes.c_int, ctypes.c_double]
    dev = torch.device("cuda:0")
    out = {"lib": a.lib, "has_mode": has_mode, "times_ms": {}, "kernels_ms": {}, "copy_ms": {}}

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

    def leg(name, m, n, N, res, B, wirings):
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
            """Profiled time of the merge stage per call (the stage both new kernels count under)."""
            if has_mode and L.baz_music_set_beam_mode(h, mode, 0.0) != 0:
                raise SystemExit("set mode")
            L.baz_music_profile(h, 1)
            for _ in range(a.steps):
                call(False)
            torch.cuda.synchronize()
            ms, cnt = ctypes.c_double(0.0), ctypes.c_uint64(0)
            L.baz_music_stage_ms(h, STAGE_MERGE, ctypes.byref(ms), ctypes.byref(cnt))
            L.baz_music_profile(h, 0)
            return ms.value / a.steps

        if L.baz_music_reserve(h, B) != 0:
            raise SystemExit("baz_music_reserve")
        for wiring in wirings:
            for mode in ((0, 1) if has_mode else (0,)):               # the modes alternate inside a round
                if has_mode:
                    if L.baz_music_set_beam_mode(h, mode, 0.0) != 0:
                        raise SystemExit("set mode")
                    L.baz_music_reserve(h, B)
                t = timed(lambda: call(wiring == "spec"))
                out["times_ms"].setdefault("%s/%s/mode%d" % (name, wiring, mode), []).append(t)
        if has_mode:
            base = merge_ms(0)
            out["kernels_ms"][name] = merge_ms(1) - base
            L.baz_music_set_beam_mode(h, 0, 0.0)
            # a plain copy of the same number of bytes (half read, half written), same process, same session
            half = B * beam_bytes(m, n, N) // 2
            src = torch.empty(half, dtype=torch.uint8, device=dev).fill_(1)
            dst = torch.empty_like(src)
            out["copy_ms"][name] = timed(lambda: dst.copy_(src))
            del src, dst
        L.baz_music_destroy(h)

    for spec_ in LEGS:
        if a.legs and spec_[0] not in a.legs.split(","):
            continue
        leg(*spec_)
        torch.cuda.empty_cache()
    print("BEAM_RATE " + json.dumps(out), flush=True)


def run_worker(lib, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    if a.legs:
        cmd += ["--legs", a.legs]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    print("worker done: %s" % lib, flush=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("BEAM_RATE ")][-1]
    return json.loads(line[len("BEAM_RATE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=OWN_LIB)
    ap.add_argument("--legs", default=None, help="comma-separated leg names (default: all)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    own, parent, kern, copy = {}, {}, {}, {}
    for rnd in range(a.rounds):                               # own library and the parent's in alternation, the order alternating too
        for which in (("own", "parent") if rnd % 2 == 0 else ("parent", "own")):
            if which == "own":
                w = run_worker(OWN_LIB, a)
                for k, v in w["times_ms"].items():
                    own.setdefault(k, []).extend(v)
                for k, v in w["kernels_ms"].items():
                    kern.setdefault(k, []).append(v)
                for k, v in w["copy_ms"].items():
                    copy.setdefault(k, []).append(v)
            elif a.parent_lib:
                w = run_worker(a.parent_lib, a)
                for k, v in w["times_ms"].items():
                    parent.setdefault(k, []).extend(v)
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))
    lines = ["Opt-in MVDR beamformer output (baz_music_set_beam_mode, DESIGN.md 8g): cost on one MI355X, one session",
             "scripts/beam_rate.py --rounds %d --steps %d --warmup %d%s" % (a.rounds, a.steps, a.warmup, " --parent-lib <parent commit's library>" if a.parent_lib else ""),
             "ms per process_device call, device-resident batch, median [min .. max] over the rounds (a fresh process per round and library, alternating)", ""]
    for name, m, n, N, res, B, wirings in LEGS:
        if a.legs and name not in a.legs.split(","):
            continue
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
            v = own["%s/%s/mode1" % (name, wiring)]
            lines.append("  this tree, mode 1    %s   %.4e items/s   x%.4f of mode 0  (+%.4f ms, %.2f ns per item)"
                         % (fmt(v), B / (statistics.median(v) * 1e-3), statistics.median(v) / statistics.median(v0),
                            statistics.median(v) - statistics.median(v0), (statistics.median(v) - statistics.median(v0)) * 1e6 / B))
        total = B * beam_bytes(m, n, N)
        k_ms, c_ms = statistics.median(kern[name]), statistics.median(copy[name])
        lines.append("  beam_weights_kernel + beam_apply_kernel (merge stage profiled, mode 1 minus mode 0): %.4f ms [%.4f .. %.4f] per call"
                     % (k_ms, min(kern[name]), max(kern[name])))
        lines.append("  beam_apply_kernel's bytes: %d B/item read + %d B/item written = %.1f MiB per call; over the time of BOTH kernels %.3f TB/s"
                     % (8 * N, 8 * n * (N // m), total / 2.0 ** 20, total / (k_ms * 1e-3) / 1e12))
        lines.append("  plain copy of the same bytes (half read, half written): %.4f ms [%.4f .. %.4f], %.3f TB/s; the two kernels reach %.3f of it"
                     % (c_ms, min(copy[name]), max(copy[name]), total / (c_ms * 1e-3) / 1e12, c_ms / k_ms))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
