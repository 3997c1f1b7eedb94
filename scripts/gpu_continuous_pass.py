"""Timing of the gradient-based continuous refinement -> profiles/continuous_pass.json (--out DIR: a copy there too).

Three figures, each step under its own time limit (a watchdog ends the process if a step overruns, so nothing more is started on the
device after a hang):

  pass       one ``bbh_posterior_grad`` + ``bbh_qlogei_partials`` pass (``HipGP.qlogei_value_grad``, the chain-rule contraction
             included) over 1 000 x 10 starts at n = 512, d_c = 8, p = 3, S = 512: median over ``--reps`` synchronised calls
  gradient   a whole ``recommend(1)`` with ``continuous_optimizer="gradient"`` at d_c = 4, 3 discrete rows x 10 starts, n = 64 (the
             fit is cached by an untimed first call): wall time of the call; its device passes are the optimiser's callback calls
  compass    the same call with ``continuous_optimizer="compass"``: the pattern search as it stood before the gradient path
             existed (this option leaves it untouched); its device passes are the posterior calls it makes

Not a gate: nothing is asserted.

Usage: python scripts/gpu_continuous_pass.py [--reps 20] [--limit SECONDS] [--out DIR]"""
import argparse
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--limit", type=float, default=120.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from baybe_amd import engine, gp_spec  # noqa: E402
from baybe_amd.recommenders import HipBotorchRecommender  # noqa: E402

record = {}


def step(name):
    faulthandler.dump_traceback_later(args.limit, exit=True)
    print(f"[{name}]", flush=True)


# ---- one derivative pass -----------------------------------------------------------------------------------------------------
step("pass")
rng = np.random.default_rng(0)
n, dd, dc, p, S = 512, 2, 8, 3, 512
d = dd + dc
Xt = rng.random((n, d))
y = -((Xt - 0.4) ** 2).sum(axis=1) + 0.01 * rng.normal(size=n)
spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
gp = engine.HipGP(0)
gp.set_model(spec, Xt, y)
gp.factorize(gp_spec.GPParams(np.full(d, 0.25 * np.sqrt(d)), 0.01, 0.0))
gp.set_pending(rng.random((p, d)))
X = torch.from_numpy(rng.random((10_000, d))).to(gp._dev())
z = engine.sobol_normal_base_samples(S, 1 + p, 5)
bf = gp.best_f(1.0)
cols = np.arange(dd, d, dtype=np.int32)
for _ in range(3):
    gp.qlogei_value_grad(X, cols, z, bf, 1.0)
torch.cuda.synchronize()
times = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    gp.qlogei_value_grad(X, cols, z, bf, 1.0)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
record["pass"] = {"N": 10_000, "n": n, "d_c": dc, "p": p, "S": S, "ms_median": statistics.median(times), "ms_all": times}
gp.set_pending(None)
gp.close()


# ---- whole refinements -------------------------------------------------------------------------------------------------------
def refinement(optimizer):
    from _replay import HybridSpace

    r = np.random.default_rng(1)
    dcr, nr = 4, 64
    disc = pd.DataFrame({"d0": [0.0, 0.5, 1.0]})
    bounds = pd.DataFrame(np.vstack([np.zeros(dcr), np.ones(dcr)]), index=["min", "max"], columns=[f"c{a}" for a in range(dcr)])
    space = HybridSpace(disc, bounds)
    M = np.hstack([r.choice([0.0, 0.5, 1.0], (nr, 1)), r.random((nr, dcr))])
    meas = pd.DataFrame(M, columns=list(space.comp_rep_columns)).assign(y=-((M - 0.4) ** 2).sum(1) + 0.01 * r.normal(size=nr))
    objective = SimpleNamespace(targets=(SimpleNamespace(name="y", minimize=False, transformation=None),), is_multi_output=False)
    rec = HipBotorchRecommender(continuous_optimizer=optimizer, n_restarts=10)
    torch.manual_seed(3)
    rec.recommend(1, space, objective, meas)  # untimed: fit, uploads, first launches
    eng = rec._surrogate_model.engine
    passes = {"n": 0}
    inner = eng.posterior

    def counted(*a, **k):
        passes["n"] += 1
        return inner(*a, **k)

    eng.posterior = counted
    torch.manual_seed(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = rec.recommend(1, space, objective, meas)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    out = {"ms": ms, "pick": got.to_numpy(dtype=float)[0].tolist()}
    if optimizer == "gradient":
        tr = rec._last_continuous_trace[0]
        out.update(device_passes=int(tr["calls"]), starts=int(len(tr["starts"])), value=float(np.nanmax(tr["values"])))
    else:
        out.update(device_passes=int(passes["n"]) - 1)  # (the first posterior call scores the raw samples)
    return out


for name in ("gradient", "compass"):
    step(name)
    record[name] = refinement(name)
faulthandler.cancel_dump_traceback_later()
print(json.dumps(record, indent=1))
for folder in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    folder.mkdir(parents=True, exist_ok=True)
    (folder / "continuous_pass.json").write_text(json.dumps(record, indent=1))
