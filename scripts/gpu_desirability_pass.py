"""Timing of one desirability scoring pass (csrc/bbh_desirability.hip) next to its yardstick -> profiles/desirability_pass.json
(--out DIR: a copy there too).

Shape: N = 1e5 and 1e6 candidates, T = 2 and 4 targets, p = 0, 3 and 7 pending points, S = 512 base samples, qLogEI, bell / ramp /
sigmoid programs under the geometric mean.  The statistics are synthetic (ordinary positive-definite rows): the pass is timed, not
the models.  Variants per (N, T, p):

  des_lds / des_ws   bbh_desirability_pending with the factors in LDS (form 0) / in the global workspace (form 1); p = 0: des_q1
  sum_obj            the sum of T passes of the EXISTING single-target kernels (bbh_mc_acq_obj_q1 / bbh_mc_acq_obj_pending) on the
                     same N, p, S - per (sample, point) the new kernel does the same draws and programs and one utility instead
                     of T, so this sum is the yardstick

A repetition is one child process that sets the inputs up, runs every variant once untimed and once event-timed; the parent starts
REPS of them one after the other, each under its own time limit, stops at the first that fails, and reports the median.  No ratio
is a requirement (KERNELS.md 4.13 records the numbers and what they say).
Usage: python scripts/gpu_desirability_pass.py [--rows N ...] [--reps K] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--limit", type=int, default=240, help="time limit of one repetition, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of desirability_pass.json")
ap.add_argument("--child", action="store_true", help="run one repetition and print its times as one JSON line")
args = ap.parse_args()
S, TARGETS, PENDING, KIND = 512, (2, 4), (0, 3, 7), "qLogEI"
PROGRAMS = ((("BELL", (0.4, 0.8)),), (("AFFINE", (-0.4, 0.6)), ("CLAMP", (0.0, 1.0))), (("SIGMOID", (0.2, 1.7)),), (("BELL", (-0.5, 1.2)),))


def repetition():
    import numpy as np
    import torch

    from baybe_amd import engine
    from baybe_amd.desirability import DesirabilityProgram
    from baybe_amd.objective import ObjectiveProgram

    g = engine.HipGP(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    times = {}
    for N in args.rows:
        for T in TARGETS:
            progs = tuple(ObjectiveProgram(ops) for ops in PROGRAMS[:T])
            des = DesirabilityProgram(progs, tuple(1.0 / T for _ in range(T)), "GEOM_MEAN")
            mean = torch.randn((T, N), dtype=torch.float64, device="cuda", generator=gen)
            for p in PENDING:
                z = engine.sobol_normal_base_samples(S, (p + 1) * T, 7).reshape(S, p + 1, T)
                if p == 0:
                    var = 0.05 + 0.5 * torch.rand((T, N), dtype=torch.float64, device="cuda", generator=gen)
                    variants = {"des_q1": lambda: g.desirability_acq(des, KIND, mean, var, z[:, 0, :], 0.5)}
                    z1 = [np.ascontiguousarray(z[:, 0, t]) for t in range(T)]
                    rows = [(mean[t].contiguous(), var[t].contiguous()) for t in range(T)]
                    variants["sum_obj"] = lambda: [g.mc_acq(KIND, rows[t][0], rows[t][1], z1[t], 0.5, objective=progs[t]) for t in range(T)]
                else:
                    B = rng.standard_normal((T, p, p + 3))
                    cpp = B @ B.transpose(0, 2, 1) / (p + 3) + 0.05 * np.eye(p)
                    mp = rng.standard_normal((T, p))
                    cross = 0.2 * torch.randn((T, N, p), dtype=torch.float64, device="cuda", generator=gen)
                    inv = torch.from_numpy(np.linalg.inv(cpp)).cuda()
                    var = (torch.einsum("tnp,tpq,tnq->tn", cross, inv, cross) + 1e-3).contiguous()  # Schur complement 1e-3: positive definite
                    variants = {f"des_{name}": (lambda form=form: g.desirability_acq(des, KIND, mean, var, z, 0.5, cross=cross, stats=(mp, cpp), form=form))
                                for name, form in (("lds", 0), ("ws", 1))}
                    zt = [np.ascontiguousarray(z[:, :, t]) for t in range(T)]
                    rows = [(mean[t].contiguous(), var[t].contiguous(), cross[t].contiguous()) for t in range(T)]
                    variants["sum_obj"] = lambda: [g.mc_acq(KIND, rows[t][0], rows[t][1], zt[t], 0.5, cross=rows[t][2], objective=progs[t],
                                                            stats=(mp[t], cpp[t])) for t in range(T)]
                for fn in variants.values():  # untimed: code objects, workspaces, allocator blocks
                    fn()
                torch.cuda.synchronize()
                for k, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    keep = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    del keep
                    times[f"N{N}-T{T}-p{p}-{k}"] = e0.elapsed_time(e1)
    g.close()
    print("TIMES " + json.dumps(times), flush=True)


if args.child:
    repetition()
    sys.exit(0)

runs, stopped = [], None
for rep in range(args.reps):
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rows", *map(str, args.rows)], capture_output=True,
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
ratio = {}
for k, v in med.items():
    head, name = k.rsplit("-", 1)
    if name != "sum_obj":
        ratio[k] = v / med[f"{head}-sum_obj"]
out = {
    "shape": {"rows": args.rows, "S": S, "targets": TARGETS, "pending": PENDING, "kind": KIND, "scalarizer": "GEOM_MEAN"},
    "repetitions": len(runs),
    "stopped": stopped,
    "median_ms": med,
    "min_ms": {k: min(r[k] for r in runs) for k in runs[0]},
    "max_ms": {k: max(r[k] for r in runs) for k in runs[0]},
    "over_sum_obj": ratio,
}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "desirability_pass.json").write_text(text + "\n")
