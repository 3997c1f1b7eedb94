"""Timing of the two polytope operations next to the pass they sit beside -> profiles/polytope_pass.json (--out DIR: a copy there too).

Three figures, each step under its own time limit (a watchdog ends the process if a step overruns, so nothing more is started on the
device after a hang):

  sample     ``bbh_polytope_sample``: R = 16 384 chains on the simplex at d_c = 32 (dz = 31), default step count (1024)
  project    one ``bbh_polytope_project`` call at k = 16 384, d_c = 32, the simplex plus one cut (c0 <= 0.1); the rows are points a
             maximiser's trial produces: feasible points moved by a step of 0.05 per coordinate
  pass       one ``HipGP.qlogei_value_grad`` pass at the same k (n = 512, 32 differentiated columns, p = 1, S = 512), the pass
             the projection sits next to in every trial of ``maximize_polytope``

Medians over ``--reps`` synchronised calls (3 for the sampler).  Not a gate: nothing is asserted.

Usage: python scripts/gpu_polytope_pass.py [--reps 20] [--limit SECONDS] [--out DIR]"""
import argparse
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--limit", type=float, default=120.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baybe_amd import engine, gp_spec  # noqa: E402
from baybe_amd.polytope import FEASIBILITY_C, Polytope, default_n_steps  # noqa: E402

record = {}
K, DC = 16_384, 32


def step(name):
    faulthandler.dump_traceback_later(args.limit, exit=True)
    print(f"[{name}]", flush=True)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


gp = engine.HipGP(0)

# ---- the sampler ---------------------------------------------------------------------------------------------------------------
step("sample")
simplex = Polytope(np.zeros(DC), np.ones(DC), np.ones((1, DC)), np.ones(1), np.zeros((0, DC)), np.zeros(0))
T = default_n_steps(simplex.dz)
times = timed(lambda: simplex.sample(gp, K, T, seed=1), 3)
record["sample"] = {"R": K, "d_c": DC, "dz": simplex.dz, "n_steps": T, "ms_median": statistics.median(times), "ms_all": times}

# ---- one projection call ---------------------------------------------------------------------------------------------------------
step("project")
cut = np.zeros((1, DC))
cut[0, 0] = -1.0
poly = Polytope(np.zeros(DC), np.ones(DC), np.ones((1, DC)), np.ones(1), cut, np.array([-0.1]))
rng = np.random.default_rng(0)
feasible = poly.sample(gp, K, seed=2)
trial = (feasible + 0.05 * torch.from_numpy(rng.normal(size=(K, DC))).to(feasible.device)).contiguous()
rows, rhs = poly.rows()
tolf = FEASIBILITY_C * (DC + poly.n_rows) * float(np.finfo(np.float64).eps)
mu_min = 1e-10 * float((rows * rows).sum(axis=1).max())
status = {}


def project():
    _, st = gp.polytope_project(trial, poly.lo, poly.hi, rows, rhs, poly.me, tolf, mu_min)
    status["bad"] = st


times = timed(project, args.reps)
record["project"] = {"k": K, "d_c": DC, "me": poly.me, "mi": poly.mi, "ms_median": statistics.median(times), "ms_all": times,
                     "status_nonzero": int((status["bad"] != 0).sum().item())}

# ---- one value-and-gradient pass at the same k ---------------------------------------------------------------------------------
step("pass")
n, dd, p, S = 512, 2, 1, 512
d = dd + DC
Xt = rng.random((n, d))
y = -((Xt - 0.4) ** 2).sum(axis=1) + 0.01 * rng.normal(size=n)
spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
gp.set_model(spec, Xt, y)
gp.factorize(gp_spec.GPParams(np.full(d, 0.25 * np.sqrt(d)), 0.01, 0.0))
gp.set_pending(rng.random((p, d)))
X = torch.cat([torch.from_numpy(rng.random((K, dd))).to(feasible.device), feasible], dim=1).contiguous()
z = engine.sobol_normal_base_samples(S, 1 + p, 5)
bf = gp.best_f(1.0)
cols = np.arange(dd, d, dtype=np.int32)
times = timed(lambda: gp.qlogei_value_grad(X, cols, z, bf, 1.0), args.reps)
record["pass"] = {"N": K, "n": n, "d_c": DC, "p": p, "S": S, "ms_median": statistics.median(times), "ms_all": times}
gp.set_pending(None)
gp.close()

faulthandler.cancel_dump_traceback_later()
print(json.dumps(record, indent=1))
for folder in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    folder.mkdir(parents=True, exist_ok=True)
    (folder / "polytope_pass.json").write_text(json.dumps(record, indent=1))
