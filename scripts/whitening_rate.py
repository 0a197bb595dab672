"""Cost of the opt-in noise pre-whitening (baz_music_set_noise_covariance) on one device, in ONE process: device-resident batches, a
hip-event pair (torch.cuda.Event) around every process_device call, the median of `--steps` calls after `--warmup` warm-ups, mode
off against mode on inside a leg.

Legs: config 2's shape (4 antennas, 1,024 samples, 3,600 bins) at 65,536 items, config 3's (8 antennas, 4,096 samples, 36,000 bins)
at 4,096 items, and the run-time-m path at 32 and 64 antennas (360 bins, 4,096 items).  Beside every time: the profiled share of the
stages (baz_music_stage_ms) over the same number of calls -- the whitening stage counts under `cov` -- and the wall time of the
setter (a retune of the table in force).

    python scripts/whitening_rate.py [--steps 20] [--warmup 5] [--out profiles/whitening.txt]

Needs a gfx950 device (no fallback)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [
    # name, m, n, nsamples, res, batch
    ("cfg2", 4, 2, 1024, 3600, 65536),
    ("cfg3", 8, 2, 4096, 36000, 4096),
    ("m32", 32, 2, 32 * 64, 360, 4096),
    ("m64", 64, 2, 64 * 64, 360, 4096),
]
STAGE_NAMES = ("cov", "evd", "scan", "merge")


def noise_covariance(m, seed=5):
    """Unequal channel powers (+-6 dB) and correlation between neighbouring channels."""
    rng = np.random.default_rng(seed)
    g = 10.0 ** (rng.uniform(-6.0, 6.0, m) / 20.0)
    C = np.eye(m, dtype=np.complex128)
    for i in range(m - 1):
        C[i + 1, i] = 0.3 * np.exp(2j * np.pi * rng.uniform())
        C[i, i + 1] = np.conj(C[i + 1, i])
    return g[:, None] * C * g[None, :] * 0.01


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
    lines = ["Opt-in noise pre-whitening (baz_music_set_noise_covariance, DESIGN.md 8j), off against on, on one MI355X, one process",
             "scripts/whitening_rate.py --steps %d --warmup %d" % (a.steps, a.warmup),
             "ms per process_device call with the spectrum port, device-resident batch: median [min .. max] of %d calls after %d warm-ups;"
             % (a.steps, a.warmup),
             "stage shares from baz_music_stage_ms over %d further calls (the whitening stage counts under cov)" % a.steps, ""]
    for name, m, n, N, res, B in LEGS:
        arr = synth.array_geometry(m)
        table = np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5, 1.0) for b in range(res)], dtype=np.complex64))
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        Rn = noise_covariance(m)
        with capi.Context(m, n, N, res, table) as ctx:
            lines.append("%s  m=%d n=%d nsamples=%d res=%d batch=%d" % (name, m, n, N, res, B))

            def call():
                ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr(), stream=stream)

            base = None
            for on in (False, True, False):
                t0 = time.perf_counter()
                ctx.set_noise_covariance(Rn if on else None)
                set_ms = (time.perf_counter() - t0) * 1e3
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
                base = med if base is None else base
                share = "  ".join("%s %.4f" % (STAGE_NAMES[s], stage[s]) for s in range(capi.NUM_STAGES))
                lines.append("  %-3s %.4f [%.4f .. %.4f] ms   %.4e items/s   x%.3f of the first off leg   setter %.3f ms   cov stage: %s   stages (ms): %s"
                             % ("on" if on else "off", med, min(times), max(times), B / (med * 1e-3), med / base, set_ms,
                                ctx.stage_name(capi.STAGE_COV), share))
            lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
