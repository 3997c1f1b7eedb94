"""Timing of the qNIPV passes (csrc/bbh_nipv.hip) next to their yardstick -> profiles/nipv_pass.json (--out DIR: a copy there too).

Shape: N = 1e5 candidates in 20 dimensions, a Matern-5/2 GP with hand-set hyper-parameters on n = 512 rows, M = 256 and 4096
integration points (rows of the candidate set), b = 0 and 4 pending points.  Per (M, b): ``nipv_set_points`` (once per
recommendation), one ``nipv_gain`` pass (operands ready: variance, cross-covariances, H and G^-1), a greedy batch of 3
(``HipNIPV.greedy``, posterior pass included), and the achieved fraction of the fp64 MFMA peak of 78.6 TFLOP/s with the pass's
flops taken as ``2 N Mpad (np + 16)``.  Every figure is the median of synchronised calls (device idle before, waited for after).

The A/B of KERNELS.md 4.15: the row tile (BBH_NIPV_TILE = 16 / 32 candidates per workgroup) and the column slicing
(BBH_NIPV_SLICE = 512 columns / 0 = one slice).  A setting is one child process (switches are read when a handle is created); the
parent starts them one after the other, each under its own time limit, and stops at the first that fails.

Yardstick (default child only): the assembly the library could already run on the same rows - ``cross_cov_many`` (ceil(M / 15)
mean-only posterior passes that materialise cov(x, P) [N, M]) + the torch reduction.  At M = 4096 the [N, M] matrix does not fit
comfortably next to the rest, so it is measured on a row subset and SCALED to N rows; the entry says so.
Usage: python scripts/gpu_nipv_pass.py [--rows N] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--limit", type=int, default=300, help="time limit of one child process, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of nipv_pass.json")
ap.add_argument("--child", action="store_true", help="run the passes under the current environment and print the times as one JSON line")
args = ap.parse_args()
D, N_TRAIN, POINTS, PENDING, REPEATS, PEAK_TFLOPS, SUBSET = 20, 512, (256, 4096), (0, 4), 7, 78.6, 8192


def passes():
    import numpy as np
    import torch

    from baybe_amd import engine, gp_spec
    from baybe_amd.nipv import HipNIPV

    rng = np.random.default_rng(0)
    Xt = rng.random((N_TRAIN, D))
    y = np.sin(3.0 * Xt.sum(1) / np.sqrt(D)) + 0.05 * rng.standard_normal(N_TRAIN)
    g = engine.HipGP(0)
    g.set_model(gp_spec.GPSpec.baybe_default(D, np.zeros(D), np.ones(D)), Xt, y)
    g.factorize(gp_spec.GPParams(np.full(D, 0.35 * np.sqrt(D)), 0.064, 0.0))
    X = torch.rand((args.rows, D), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    Xh = X.cpu().numpy()
    N = args.rows
    default = not any(k in os.environ for k in ("BBH_NIPV_TILE", "BBH_NIPV_SLICE"))
    times = {}

    def median_ms(fn, repeats=REPEATS):
        fn()  # untimed: code objects, workspaces
        ms = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            del keep
        return statistics.median(ms)

    for M in POINTS:
        P = Xh[1000:1000 + M]
        hn = HipNIPV(g, P)
        times[f"set_points-M{M}"] = median_ms(lambda: g.nipv_set_points(P), 3)
        hn._prepare()
        Mpad = -(-M // 64) * 64
        for b in PENDING:
            pend = Xh[5000:5000 + b]
            Xd, var = hn._variance(X)
            H, ginv, _ = hn.conditioning_terms(pend)
            cross = g.cross_cov(Xd) if b else None
            ms = median_ms(lambda: g.nipv_gain(Xd, var, cross, H, ginv))
            times[f"gain-M{M}-b{b}"] = ms
            times[f"gain-M{M}-b{b}-form"] = g.nipv_last_form()
            times[f"gain-M{M}-b{b}-mfma_fraction"] = 2.0 * N * Mpad * (512 + 16) / (ms * 1e-3) / (PEAK_TFLOPS * 1e12)
            g.set_pending(None)
            if default:
                times[f"greedy3-M{M}-b{b}"] = median_ms(lambda: hn.greedy(X, 3, seed=0, X_pending=pend), 3)
                rows = N if M <= 256 else min(N, SUBSET)
                Xs = X[:rows].contiguous()
                s2 = hn.s2

                def yardstick():
                    g.set_pending(None)
                    v = g.posterior(Xs)[1]
                    C = g.cross_cov_many(Xs, P)
                    if b:
                        _, cpp = g.set_pending(pend)
                        cb = g.cross_cov(Xs)
                        C = C - cb @ torch.from_numpy(H).to(C.device)
                        gi = torch.from_numpy(ginv).to(C.device)
                        v = torch.clamp(v - ((cb @ gi) * cb).sum(1), min=0.0)
                    return (C * C).sum(1) / (v + s2)

                yms = median_ms(yardstick, 3)
                times[f"yardstick-M{M}-b{b}"] = yms * (N / rows)
                times[f"yardstick-M{M}-b{b}-note"] = ("measured on all rows" if rows == N else
                                                      f"measured on {rows} rows ({yms:.2f} ms) and scaled by {N / rows:.3f} to {N} rows")
                g.set_pending(None)
    g.close()
    print("TIMES " + json.dumps(times), flush=True)


if args.child:
    passes()
    sys.exit(0)

SETTINGS = (("default", {}), ("tile16", {"BBH_NIPV_TILE": "16"}), ("tile32", {"BBH_NIPV_TILE": "32"}),
            ("tile16_one_slice", {"BBH_NIPV_TILE": "16", "BBH_NIPV_SLICE": "0"}), ("tile32_one_slice", {"BBH_NIPV_TILE": "32", "BBH_NIPV_SLICE": "0"}))
results, stopped = {}, None
for label, extra in SETTINGS:
    env = dict(os.environ)
    env.pop("BBH_NIPV_TILE", None)
    env.pop("BBH_NIPV_SLICE", None)
    env.update(extra)
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rows", str(args.rows)], capture_output=True, text=True,
                           timeout=args.limit, env=env)
    except subprocess.TimeoutExpired:
        stopped = f"{label}: time limit of {args.limit} s"
        break
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")]
    if r.returncode != 0 or not line:
        stopped = f"{label}: exit status {r.returncode}: {r.stderr[-600:]}"
        break  # nothing more is started on the device after a failure
    results[label] = json.loads(line[0][6:])
    print(label, json.dumps(results[label], indent=1), flush=True)
if not results:
    sys.exit(f"no child finished: {stopped}")
out = {"shape": {"rows": args.rows, "d": D, "train_rows": N_TRAIN, "points": POINTS, "pending": PENDING, "repeats": REPEATS,
                 "peak_tflops": PEAK_TFLOPS},
       "stopped": stopped, "ms": results}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "nipv_pass.json").write_text(text + "\n")
