"""Timing of the exact Shapley passes (csrc/bbh_shap.hip) -> profiles/shap_pass.json (--out DIR: a copy there too).

Shape: R = 128 explained rows and B = 128 background rows in d = 12 columns forming M = 10 features (one group of three columns,
nine single columns), a Matern-5/2 GP with hand-set hyper-parameters on n = 128 rows: R 2^M B n = 2.1e9 kernel values.  Timed on the
same inputs: the fused form (``bbh_shap_values``; one and four coalitions per thread, BBH_SHAP_CPT, next to the default's choice)
and the composed form (``bbh_shap_compose`` -> ``bbh_posterior`` -> ``bbh_shap_reduce`` -> ``bbh_shap_apply`` in chunks of 64 MiB of
composed rows).  Every figure is the median of synchronised calls; kernel values per second = R 2^M B n / time.  The largest
difference of the two forms' phi is recorded next to the times.  A setting is one child process (switches are read when a handle
is created); the parent starts them one after the other, each under its own time limit, and stops at the first that fails.

--oracle K: no device - the numpy oracle of tests/_oracle_shap.py on the same inputs for the first K explained rows, timed on the
host and scaled to R rows (the only host comparison available without the ``shap`` package).
Usage: python scripts/gpu_shap_pass.py [--limit SECONDS] [--out DIR] | --oracle K"""
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
ap.add_argument("--limit", type=int, default=240, help="time limit of one child process, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of shap_pass.json")
ap.add_argument("--child", action="store_true", help="run the passes under the current environment and print the times as one JSON line")
ap.add_argument("--oracle", type=int, default=0, help="time the numpy oracle on the host for this many explained rows")
args = ap.parse_args()
R, B, N_TRAIN, D, M, REPEATS = 128, 128, 128, 12, 10, 5
GROUPS = [0, 0, 0] + list(range(1, 10))


def inputs():
    import numpy as np

    rng = np.random.default_rng(0)
    Xt = rng.random((N_TRAIN, D))
    y = np.sin(3.0 * Xt.sum(1) / np.sqrt(D)) + 0.05 * rng.standard_normal(N_TRAIN)
    return Xt, y, rng.random((R, D)), rng.random((B, D)), np.full(D, 0.35 * np.sqrt(D)), 0.016, 0.0


def oracle(rows):
    import numpy as np

    sys.path.insert(0, str(ROOT / "tests"))
    import _oracle_shap as osh
    from oracle import gp_oracle as go

    Xt, y, X, Bg, ls, noise, mean = inputs()
    om = go.fit_gp(go.GPSpec.baybe_default(D, np.zeros(D), np.ones(D)), Xt, y, go.GPParams(ls, noise, mean))
    t0 = time.perf_counter()
    osh.explain(om, X[:rows], Bg, np.array(GROUPS), M)
    s = time.perf_counter() - t0
    print(json.dumps({"oracle_rows": rows, "seconds": s, "scaled_to_R_rows_seconds": s * R / rows}))


def passes():
    import numpy as np
    import torch

    from baybe_amd import engine, gp_spec

    Xt, y, X, Bg, ls, noise, mean = inputs()
    g = engine.HipGP(0)
    g.set_model(gp_spec.GPSpec.baybe_default(D, np.zeros(D), np.ones(D)), Xt, y)
    g.factorize(gp_spec.GPParams(ls, noise, mean))
    Xd, Bd = torch.from_numpy(X).cuda(), torch.from_numpy(Bg).cuda()
    groups = np.array(GROUPS, dtype=np.int32)
    default = "BBH_SHAP_CPT" not in os.environ
    values = float(R) * (1 << M) * B * N_TRAIN
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

    ms = median_ms(lambda: g.shap_values(Xd, Bd, groups, form="fused"))
    times["fused_ms"], times["fused_kernel_values_per_s"] = ms, values / (ms * 1e-3)
    if default:
        ms = median_ms(lambda: g.shap_values(Xd, Bd, groups, form="composed"), 3)
        times["composed_ms"], times["composed_kernel_values_per_s"] = ms, values / (ms * 1e-3)
        a, b = g.shap_values(Xd, Bd, groups, form="fused")[0], g.shap_values(Xd, Bd, groups, form="composed")[0]
        times["max_abs_phi_difference"] = float((a - b).abs().max())
        times["max_abs_phi"] = float(a.abs().max())
    g.close()
    print("TIMES " + json.dumps(times), flush=True)


if args.oracle:
    oracle(args.oracle)
    sys.exit(0)
if args.child:
    passes()
    sys.exit(0)

SETTINGS = (("default", {}), ("cpt1", {"BBH_SHAP_CPT": "1"}), ("cpt4", {"BBH_SHAP_CPT": "4"}))
results, stopped = {}, None
for label, extra in SETTINGS:
    env = dict(os.environ)
    env.pop("BBH_SHAP_CPT", None)
    env.update(extra)
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], capture_output=True, text=True, timeout=args.limit, env=env)
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
out = {"shape": {"R": R, "B": B, "train_rows": N_TRAIN, "d": D, "M": M, "repeats": REPEATS, "kernel_values": float(R) * (1 << M) * B * N_TRAIN},
       "stopped": stopped, "ms": results}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "shap_pass.json").write_text(text + "\n")
