"""Cost of the opt-in wideband (subband) mode (baz_music_set_subbands) on one device, in ONE process: device-resident batches, a hip-event
pair (torch.cuda.Event) around every call, the median of `--steps` calls after `--warmup` warm-ups; the same context with the mode off
against the mode on, the channeliser alone (debug_subbands) beside a plain device-to-device copy of the same bytes, and the combine
alone (debug_subband_combine).

Legs: (m 4, K 256, res 3600) and (m 8, K 512, res 360), each with F = 8 and the S = 7 subbands within 75 % of the band.

    python scripts/subband_rate.py [--steps 20] [--warmup 5] [--out profiles/subband.txt]

Needs a gfx950 device (no fallback)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [
    # name, m, n, K, res, batch, F
    ("m4", 4, 2, 256, 3600, 4096, 8),
    ("m8", 8, 2, 512, 360, 4096, 8),
]
FS_OVER_FC, OCCUPIED = 0.4, 0.75


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
    from gr_baz_amd.baz import music_doa_helper as helper
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()          # (a stream of its own: the context launches on it, the events are recorded on it)
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    lines = ["Opt-in wideband (subband) MUSIC (baz_music_set_subbands, DESIGN.md 8l), off against on, on one MI355X, one process",
             "scripts/subband_rate.py --steps %d --warmup %d" % (a.steps, a.warmup),
             "ms per process_device call with the spectrum port, device-resident batch: median [min .. max] of %d calls after %d warm-ups;"
             % (a.steps, a.warmup),
             "channeliser: subband_kernel alone (debug_subbands) on the same batch, beside a device-to-device copy of as many bytes as it",
             "reads and writes; combine: subband_combine_kernel alone (debug_subband_combine) on the batch's S spectra; the same way", ""]
    for name, m, n, K, res, B, F in LEGS:
        N = m * K
        arr = synth.array_geometry(m)

        def table_at(scale):              # (the wavelength in units of the centre's: the array is 0.5 centre wavelengths apart)
            return np.ascontiguousarray(np.array([synth.steering(b * 360.0 / res, arr, 0.5 / scale, 1.0) for b in range(res)], dtype=np.complex64))

        table = table_at(1.0)
        bins = helper.subband_bins(F, OCCUPIED)
        S = len(bins)
        tabs = np.stack([table_at(1.0 / (1.0 + helper.subband_offset(k, F) * FS_OVER_FC / F)) for k in bins])
        x = synth.synth_stream(torch, dev, B, m, N, arr, synth.C_LIGHT, 0.5, snr_db=20.0, seed=7)
        ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=dev)
        y = torch.zeros(S * B * (K // F) * m * 2, dtype=torch.float32, device=dev)
        ps = torch.rand(S * B * res, dtype=torch.float32, device=dev) + 0.5
        moved = B * K * m * 8 + S * B * (K // F) * m * 8             # bytes the channeliser reads + writes
        src = torch.zeros(moved // 2 // 4, dtype=torch.float32, device=dev)
        dst = torch.zeros_like(src)
        with capi.Context(m, n, N, res, table) as ctx:
            lines.append("%s  m=%d n=%d K=%d res=%d batch=%d  F=%d S=%d bins %s" % (name, m, n, K, res, B, F, S, bins))

            def call():
                ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr(), stream=stream)

            ctx.set_stream(stream)
            base = None
            for on in (False, True, False):
                if on:
                    ctx.set_subbands(F, bins, tabs)
                else:
                    ctx.set_subbands(None)
                ctx.reserve(B)
                med, lo_t, hi_t = timed(torch, call, a.steps, a.warmup)
                base = med if base is None else base
                lines.append("  %-3s %.4f [%.4f .. %.4f] ms   %.4e items/s   x%.3f of the first off leg"
                             % ("on" if on else "off", med, lo_t, hi_t, B / (med * 1e-3), med / base))
                if on:
                    cm, cl, ch = timed(torch, lambda: ctx.debug_subbands(x.data_ptr(), B, y.data_ptr()), a.steps, a.warmup)
                    pm, pl, ph = timed(torch, lambda: dst.copy_(src), a.steps, a.warmup)
                    lines.append("      channeliser alone %.4f [%.4f .. %.4f] ms   %.1f GB/s of input + output (%.1f MB)"
                                 % (cm, cl, ch, moved / 1e9 / (cm * 1e-3), moved / 1e6))
                    lines.append("      device copy       %.4f [%.4f .. %.4f] ms   %.1f GB/s of read + write (the same bytes)"
                                 % (pm, pl, ph, moved / 1e9 / (pm * 1e-3)))
                    bm, bl, bh = timed(torch, lambda: ctx.debug_subband_combine(ps.data_ptr(), B, spec.data_ptr()), a.steps, a.warmup)
                    cb = (S + 1) * B * res * 4
                    lines.append("      combine alone     %.4f [%.4f .. %.4f] ms   %.1f GB/s of input + output (%.1f MB)"
                                 % (bm, bl, bh, cb / 1e9 / (bm * 1e-3), cb / 1e6))
                    # a plain call at K / F snapshots, for the "S plain calls" reading
                    with capi.Context(m, n, m * (K // F), res, tabs[0]) as small:
                        small.set_stream(stream)
                        small.reserve(B)
                        sm_, sl, sh = timed(torch, lambda: small.process_device(y.data_ptr(), B, ang.data_ptr(), None, spec.data_ptr(),
                                                                                 stream=stream), a.steps, a.warmup)
                    lines.append("      one plain call at K / F = %d snapshots %.4f [%.4f .. %.4f] ms   (x S = %.4f ms)"
                                 % (K // F, sm_, sl, sh, S * sm_))
            lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
