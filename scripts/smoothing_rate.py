"""Throughput of the opt-in forward-backward averaging / spatial smoothing mode (baz_music_set_smoothing) against the plain
engine on the same batch, device-resident, timed with hip events (torch.cuda.Event) around `--steps` back-to-back calls.

    python scripts/smoothing_rate.py [--steps 20] [--warmup 3] [--json OUT]

Legs: FB only at config 2's shape (4-element unit square, n = 2, 1,024 samples, 3,600 bins) and FB + SS over 6-element
subarrays at config 3's shape on an 8-element ULA (config 3's own circle is not shift invariant; n = 2, 4,096 samples,
36,000 bins), spectrum port wired.  The expectation is roughly plain throughput / (2 L m_s / m), the byte ratio of a
re-stacked item.  Prints one JSON line per leg; needs a gfx950 device (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [
    # name, array kind, m, n, nsamples, res, batch, subarray, forward-backward
    ("cfg2_fb", "square", 4, 2, 1024, 3600, 16384, 4, True),
    ("cfg3_ula_fb_ss6", "ula", 8, 2, 4096, 36000, 1024, 6, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 device")
    from gr_baz_amd import capi, synth
    dev = torch.device("cuda:0")
    freq, spacing = synth.C_LIGHT, 0.5          # lambda = 1 m, half-wavelength spacing
    rows = []
    for name, kind, m, n, N, res, B, ms, fb in LEGS:
        arr = synth.array_geometry(4) if kind == "square" else [[i, 0] for i in range(m)]
        table = np.array([synth.steering(b * 360.0 / res, arr, spacing, 1.0) for b in range(res)], dtype=np.complex64)
        x = synth.synth_stream(torch, dev, B, m, N, arr, freq, spacing, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        row = {"leg": name, "m": m, "n": n, "nsamples": N, "res": res, "batch": B, "subarray": ms, "forward_backward": fb}
        with capi.Context(m, n, N, res, table, device_id=0) as ctx:
            for mode in ("plain", "smoothed"):
                ctx.set_smoothing(ms, fb) if mode == "smoothed" else ctx.set_smoothing(m, False)
                ctx.reserve(B)
                stream = torch.cuda.current_stream().cuda_stream
                for _ in range(a.warmup):
                    ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr(), stream=stream)
                e1.record()
                torch.cuda.synchronize()
                ms_call = e0.elapsed_time(e1) / a.steps
                row[mode + "_ms_per_call"] = round(ms_call, 4)
                row[mode + "_items_per_s"] = round(B / (ms_call * 1e-3), 1)
        L = m - ms + 1
        K = N // m
        Kp = L * K * (2 if fb else 1)
        row["restack_bytes_per_item"] = 8 * N + 8 * ms * Kp         # read the item once, write the re-stacked item
        row["byte_ratio_2Lms_over_m"] = round((2 if fb else 1) * L * ms / m, 3)
        row["slowdown"] = round(row["smoothed_ms_per_call"] / row["plain_ms_per_call"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
