"""Cost of the dominance check that follows the orthogonal iteration (evd_sub_kernel, sub_wide_kernel): the EVD
stage's own time (baz_music_stage_ms, hip events around the stage's kernels) of this tree against a checkout of the PARENT
commit built beside it, at 16 and 32 antennas with 2 emitters, a few thousand 20 dB items, device-resident.

    python scripts/evd_dominance_rate.py --parent-root PATH [--rounds 3] [--steps 40] [--warmup 10] > profiles/evd_dominance_check.txt

Every (tree, round) runs in a fresh child process (this file with --worker, started in that tree), one at a time, the two
trees alternating, the parent first: the parent's own rounds give its run-to-run spread.  Needs a gfx950 device (no fallback)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 2, 64, 360, 4096), (32, 2, 64, 360, 4096)]       # m, n, K, res, items
STAGE_EVD = 1


def scene(m, K, res, B, angles_deg=(40.3, 121.7), snr_db=20.0, seed=5):
    """steering table (res, m) and B items of two unit-power complex-Gaussian emitters plus white noise, complex64"""
    import numpy as np
    from gr_baz_amd import synth
    arr = synth.array_geometry(m)
    table = np.array([synth.steering(b * 360.0 / res, arr, 0.5, 1.0) for b in range(res)]).astype(np.complex64)
    rng = np.random.default_rng(seed)
    x = np.zeros((B, K, m), dtype=np.complex128)
    for th in angles_deg:
        s = (rng.standard_normal((B, K)) + 1j * rng.standard_normal((B, K))) / np.sqrt(2.0)
        x += s[:, :, None] * synth.steering(th, arr, 0.5, 1.0)[None, None, :]
    noise = (rng.standard_normal((B, K, m)) + 1j * rng.standard_normal((B, K, m))) / np.sqrt(2.0)
    x += 10.0 ** (-snr_db / 20.0) * noise
    return np.ascontiguousarray(table), x.reshape(B, K * m).astype(np.complex64)


def worker(a):
    sys.path.insert(0, os.getcwd())
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a gfx950 device")
    from gr_baz_amd import capi
    dev = torch.device("cuda:0")
    out = {}
    for (m, n, K, res, B) in SHAPES:
        table, items = scene(m, K, res, B)
        with capi.Context(m, n, m * K, res, table) as ctx:
            x = torch.from_numpy(items.view(np.float32)).to(dev)
            ang = torch.zeros(B, n, dtype=torch.float32, device=dev)
            lvl = torch.zeros_like(ang)
            torch.cuda.synchronize()
            ctx.profile(1)

            def step():
                ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), None, stream=torch.cuda.current_stream().cuda_stream)
            for _ in range(a.warmup):
                step()
            t0, c0 = ctx.stage_ms(STAGE_EVD)
            for _ in range(a.steps):
                step()
            t1, c1 = ctx.stage_ms(STAGE_EVD)
            out["m%d_n%d" % (m, n)] = (t1 - t0) / max(1, a.steps)
            out["m%d_n%d_launches" % (m, n)] = int(c1 - c0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-root")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root:
        raise SystemExit("--parent-root: a checkout of the parent commit with its libraries built")
    runs = {"parent": [], "this": []}
    for r in range(a.rounds):
        for name, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               cwd=root, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                                 # nothing more is started on the device after a failed child
                sys.stderr.write(p.stderr)
                raise SystemExit("worker of the %s tree failed with status %d" % (name, p.returncode))
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print("# EVD stage (baz_music_stage_ms, ms per call of %d items), %d steps after %d warm-up calls, rounds alternating parent / this tree"
          % (SHAPES[0][4], a.steps, a.warmup))
    for (m, n, K, res, B) in SHAPES:
        k = "m%d_n%d" % (m, n)
        pv = [r[k] for r in runs["parent"]]
        tv = [r[k] for r in runs["this"]]
        print("m = %d, n = %d, K = %d, %d items" % (m, n, K, B))
        print("  parent rounds: " + "  ".join("%.4f" % v for v in pv) + "   median %.4f  spread %.4f .. %.4f" % (statistics.median(pv), min(pv), max(pv)))
        print("  this   rounds: " + "  ".join("%.4f" % v for v in tv) + "   median %.4f  spread %.4f .. %.4f" % (statistics.median(tv), min(tv), max(tv)))
        d = statistics.median(tv) / statistics.median(pv) - 1.0
        print("  this / parent (medians): %+.1f %%; inside the parent's own spread: %s" % (100.0 * d, min(pv) <= statistics.median(tv) <= max(pv)))


if __name__ == "__main__":
    main()
