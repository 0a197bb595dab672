"""Cost of the opt-in beamspace mode (baz_music_set_beamspace) on one device, in ONE process: device-resident batches, a hip-event pair
(torch.cuda.Event) around every process_device call, the median of `--steps` calls after `--warmup` warm-ups; the same context with
the mode off (the run-time-m path at that antenna count) against the mode on, and the projection kernel alone (debug_beamspace).

Legs: 4,096 items, 360 bins, 64 snapshots, at 32 -> 16 and 64 -> 16 beams (T: the sector [20, 140) resp. [20, 80) of the table).

    python scripts/beamspace_rate.py [--steps 20] [--warmup 5] [--out profiles/beamspace.txt]

Needs a gfx950 device (no fallback)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [
    # name, m, n, K, res, batch, beams, first bin, bins
    ("m32->16", 32, 2, 64, 360, 4096, 16, 20, 120),
    ("m64->16", 64, 2, 64, 360, 4096, 16, 20, 60),
]


def timed(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 device")
    from gr_baz_amd import capi, synth
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()          # (a stream of its own: the context launches on it, the events are recorded on it)
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    lines = ["Opt-in beamspace MUSIC (baz_music_set_beamspace, DESIGN.md 8k), off (the run-time-m path) against on, on one MI355X, one process",
             "scripts/beamspace_rate.py --steps %d --warmup %d" % (a.steps, a.warmup),
             "ms per process_device call with the spectrum port, device-resident batch: median [min .. max] of %d calls after %d warm-ups;"
             % (a.steps, a.warmup),
             "projection: beamspace_kernel alone (debug_beamspace) on the same batch, the same way", ""]
    for name, m, n, K, res, B, beams, lo, cnt in LEGS:
        N = m * K
        arr = synth.array_geometry(m)
        table = np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5, 1.0) for b in range(res)], dtype=np.complex64))
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        y = torch.zeros(B * K * beams * 2, dtype=torch.float32, device=dev)
        T, captured = capi.beamspace_design(table, lo, cnt, beams)
        with capi.Context(m, n, N, res, table) as ctx:
            lines.append("%s  m=%d n=%d K=%d res=%d batch=%d  beams=%d sector [%d, %d) captured %.5f"
                         % (name, m, n, K, res, B, beams, lo, lo + cnt, captured))

            def call():
                ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr(), stream=stream)

            ctx.set_stream(stream)

            def project():
                ctx.debug_beamspace(x.data_ptr(), B, y.data_ptr())

            base = None
            for on in (False, True, False):
                ctx.set_beamspace(T if on else None)
                ctx.reserve(B)
                med, lo_t, hi_t = timed(torch, call, a.steps, a.warmup)
                base = med if base is None else base
                lines.append("  %-3s %.4f [%.4f .. %.4f] ms   %.4e items/s   x%.3f of the first off leg"
                             % ("on" if on else "off", med, lo_t, hi_t, B / (med * 1e-3), med / base))
                if on:
                    pm, pl, ph = timed(torch, project, a.steps, a.warmup)
                    gb = (B * K * (m + beams) * 8) / 1e9
                    lines.append("      projection alone %.4f [%.4f .. %.4f] ms   %.1f GB/s of input + output" % (pm, pl, ph, gb / (pm * 1e-3)))
            lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
