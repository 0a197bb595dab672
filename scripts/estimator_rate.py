"""Rate of the opt-in Capon and Bartlett spectrum estimators (baz_music_set_estimator) against MUSIC on one device, in ONE process:
device-resident batches, a hip-event pair (torch.cuda.Event) around every process_device call, the median of `--steps` calls after
`--warmup` warm-ups, the kinds alternating inside a leg.

Legs: config 2's shape (4 antennas, 1,024 samples, 3,600 bins) at 65,536 items and config 3's (8 antennas, 4,096 samples, 36,000
bins) at 4,096 items, each with and without the spectrum port.  Beside every time: the profiled share of the stages
(baz_music_stage_ms) over the same number of calls, and the spectrum bytes per second the scan stage alone sustains.

    python scripts/estimator_rate.py [--steps 20] [--warmup 5] [--out profiles/estimator_mode.txt]

Needs a gfx950 device (no fallback)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [
    # name, m, n, nsamples, res, batch
    ("cfg2", 4, 2, 1024, 3600, 65536),
    ("cfg3", 8, 2, 4096, 36000, 4096),
]
KIND_NAMES = {0: "MUSIC", 1: "Capon", 2: "Bartlett"}
STAGE_NAMES = ("cov", "evd", "scan", "merge")


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
    stream = torch.cuda.current_stream().cuda_stream
    lines = ["Opt-in Capon / Bartlett spectrum estimators (baz_music_set_estimator, DESIGN.md 8i) against MUSIC on one MI355X, one process",
             "scripts/estimator_rate.py --steps %d --warmup %d" % (a.steps, a.warmup),
             "ms per process_device call, device-resident batch: median [min .. max] of %d calls after %d warm-ups; stage shares from"
             % (a.steps, a.warmup),
             "baz_music_stage_ms over %d further calls; 'scan GB/s': spectrum bytes written per second of the scan stage alone" % a.steps, ""]
    for name, m, n, N, res, B in LEGS:
        arr = synth.array_geometry(m)
        table = np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5, 1.0) for b in range(res)], dtype=np.complex64))
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        with capi.Context(m, n, N, res, table) as ctx:
            for wired in (True, False):
                lines.append("%s  m=%d n=%d nsamples=%d res=%d batch=%d  spectrum port %s"
                             % (name, m, n, N, res, B, "wired" if wired else "not wired (the scan writes the private spectrum)"))

                def call():
                    ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr() if wired else None, stream=stream)

                base = None
                for kind in (0, 1, 2):
                    ctx.set_estimator(kind)
                    ctx.reserve(B)
                    for _ in range(a.warmup):
                        call()
                    torch.cuda.synchronize()
                    times = []
                    for _ in range(a.steps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call()
                        e1.record()
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1))
                    ctx.profile(1)
                    for _ in range(a.steps):
                        call()
                    stage = [ctx.stage_ms(s)[0] / a.steps for s in range(capi.NUM_STAGES)]
                    ctx.profile(0)
                    med = statistics.median(times)
                    base = med if kind == 0 else base
                    share = "  ".join("%s %.4f" % (STAGE_NAMES[s], stage[s]) for s in range(capi.NUM_STAGES))
                    lines.append("  kind %d %-8s %.4f [%.4f .. %.4f] ms   %.4e items/s   x%.3f of MUSIC   stages (ms): %s   scan share %.0f %%   scan GB/s %.0f"
                                 % (kind, KIND_NAMES[kind], med, min(times), max(times), B / (med * 1e-3), med / base, share,
                                    100.0 * stage[capi.STAGE_SCAN] / max(sum(stage), 1e-12),
                                    4.0 * res * B / (stage[capi.STAGE_SCAN] * 1e-3) / 1e9))
                ctx.set_estimator(0)
                lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
