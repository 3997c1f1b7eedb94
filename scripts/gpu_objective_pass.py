"""Timing of the objective-program scoring passes (csrc/bbh_objacq.hip) next to the kernels of the untransformed path on the same
inputs -> profiles/objective_pass.json (--out DIR: a copy there too).

Shape: 1e6 candidates (d = 3, n = 32 training points - the model only supplies mean / variance / cross-covariances), S = 512 base
samples, a bell program.  Variants, for qLogEI and qEI each:

  obj_q1 / sign_q1   bbh_mc_acq_obj_q1 against bbh_mc_acq_q1                      (q' = 1)
  obj_p4 / sign_p4   bbh_mc_acq_obj_pending against bbh_mc_acq_pending, p = 4     (q' = 5: the LDS form against the register form)

A repetition is one child process that sets the inputs up, runs every variant once untimed and once event-timed, alternating the
two sides; the parent starts REPS of them one after the other, each under its own time limit, stops at the first that fails, and
reports the median over the repetitions.  No ratio is a requirement: the numbers say whether register-resident instantiations and
sample slices for the objective kernels are worth building (KERNELS.md).
Usage: python scripts/gpu_objective_pass.py [--rows N] [--reps K] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit", type=int, default=180, help="time limit of one repetition, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of objective_pass.json")
ap.add_argument("--child", action="store_true", help="run one repetition and print its times as one JSON line")
args = ap.parse_args()
S, P, D, N_TRAIN = 512, 4, 3, 32
KINDS = ("qLogEI", "qEI")


def repetition():
    import numpy as np
    import torch

    from baybe_amd import engine, gp_spec
    from baybe_amd.objective import ObjectiveProgram

    N = args.rows
    rng = np.random.default_rng(0)
    X = rng.random((N, D))
    Xt = rng.random((N_TRAIN, D))
    y = Xt.sum(1) - 0.8 + 0.3 * np.sin(3 * Xt[:, 0]) + 0.02 * rng.standard_normal(N_TRAIN)
    g = engine.HipGP(0)
    g.set_model(gp_spec.GPSpec.baybe_default(D, np.zeros(D), np.ones(D)), Xt, y)
    g.factorize(gp_spec.GPParams(np.full(D, 0.6), 0.01, 0.0))  # (fixed hyper-parameters: the passes are timed, not the fit)
    Xd = torch.from_numpy(X).cuda()
    mean, var = g.posterior(Xd)
    stats = g.set_pending(rng.random((P, D)))
    cross = g.cross_cov(Xd)
    prog = ObjectiveProgram((("BELL", (0.4, 0.3)),))
    z1 = engine.sobol_normal_base_samples(S, 1, 7)[:, 0]
    zq = engine.sobol_normal_base_samples(S, 1 + P, 7)
    bf_sign, bf_obj = g.best_f(1.0), g.best_f(1.0, prog)
    variants = {}
    for kind in KINDS:
        variants[f"obj_q1[{kind}]"] = lambda kind=kind: g.mc_acq(kind, mean, var, z1, bf_obj, objective=prog)
        variants[f"sign_q1[{kind}]"] = lambda kind=kind: g.mc_acq(kind, mean, var, z1, bf_sign, 1.0)
        variants[f"obj_p4[{kind}]"] = lambda kind=kind: g.mc_acq(kind, mean, var, zq, bf_obj, cross=cross, objective=prog, stats=stats)
        variants[f"sign_p4[{kind}]"] = lambda kind=kind: g.mc_acq(kind, mean, var, zq, bf_sign, 1.0, cross=cross)
    for fn in variants.values():  # untimed: code objects, workspaces, allocator blocks
        fn()
    torch.cuda.synchronize()
    times = {}
    for k, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[k] = e0.elapsed_time(e1)
    g.close()
    print("TIMES " + json.dumps(times), flush=True)


if args.child:
    repetition()
    sys.exit(0)

runs, stopped = [], None
for rep in range(args.reps):
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rows", str(args.rows)], capture_output=True,
                           text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        stopped = f"repetition {rep}: time limit of {args.limit} s"
        break
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")]
    if r.returncode != 0 or not line:
        stopped = f"repetition {rep}: exit status {r.returncode}: {r.stderr[-400:]}"
        break  # nothing more is started on the device after a failure
    runs.append(json.loads(line[0][6:]))
if not runs:
    sys.exit(f"no repetition finished: {stopped}")
med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
out = {
    "shape": {"rows": args.rows, "d": D, "n_train": N_TRAIN, "S": S, "pending": P, "program": "BELL(0.4, 0.3)"},
    "repetitions": len(runs),
    "stopped": stopped,
    "median_ms": med,
    "min_ms": {k: min(r[k] for r in runs) for k in runs[0]},
    "max_ms": {k: max(r[k] for r in runs) for k in runs[0]},
    "obj_over_sign": {f"{w}[{kind}]": med[f"obj_{w}[{kind}]"] / med[f"sign_{w}[{kind}]"] for w in ("q1", "p4") for kind in KINDS},
}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "objective_pass.json").write_text(text + "\n")
