"""Timing of one qLogNEI scoring pass at the single-target headline shape (1e6 x 20 candidates, n = 512 training points, S = 512
base samples, pruned baseline) -> profiles/nei_pass.json (--out DIR: a copy there too).  Warm-up, then the median of REPS
event-timed passes of

  (a) the fused scoring pass (bbh_score_nei: conditional means contracted and scored in registers);
  (b) bbh_posterior_columns_sm alone on the same extended model: the same contraction + the [S, N] store (4.1 GB);
  (c) the chunked unfused form (bbh_posterior_columns_sm + bbh_nei_q1 over chunks of 65 536 candidates);
  (d) one fused qLogEI step on the un-extended model, for context.

All four are timed directly, without the extended model's variance pass; (a) and (c) are also given with it, i.e. as
HipNEI.score runs them.  The variants alternate inside
every repetition.  Usage: python scripts/gpu_nei_pass.py [--rows N] [--reps K] [--out DIR]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from baybe_amd import engine, gp_spec  # noqa: E402
from baybe_amd.nei import HipNEI  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out", default=None, help="directory that receives a second copy of nei_pass.json")
args = ap.parse_args()
N, d, n, S = args.rows, 20, 512, 512

rng = np.random.default_rng(0)
X = rng.integers(0, 11, size=(N, d)) / 10.0
Xt = rng.integers(0, 11, size=(n, d)) / 10.0
Xt = Xt[np.sort(np.unique(Xt, axis=0, return_index=True)[1])]
y = -((Xt - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(len(Xt))
spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
g = engine.HipGP(0)
g.set_model(spec, Xt, y)
g.factorize(gp_spec.GPParams(np.full(d, 1.5), 0.02, 0.0))  # (fixed hyper-parameters: the passes are timed, not the fit)
Xd = torch.from_numpy(X).cuda()

scorers = {}
for fused in ("1", "0"):  # a handle reads its switches when it is created
    os.environ["BBH_NEI_FUSED"] = fused
    hv = HipNEI(g, 1.0, Xt, n_mc_samples=S, prune_baseline=True)
    hv.prepare(7, prune_seed=8)
    scorers[fused] = hv
os.environ.pop("BBH_NEI_FUSED")
hf, hu = scorers["1"], scorers["0"]
ext = hf.outputs[0].ext
lib = hf._lib
zx = hf.zx.ctypes.data_as(engine._lib.c_double_p)
_, var = ext.posterior(Xd)
scores = torch.empty(N, dtype=torch.float64, device=Xd.device)
tmat = torch.empty((S, N), dtype=torch.float64, device=Xd.device)
z1 = engine.sobol_normal_base_samples(S, 1, 7)[:, 0]
best_f = g.best_f(1.0)


def fused_only():
    rc = lib.bbh_score_nei(ext._h, hf.kind, Xd.data_ptr(), N, Xd.stride(0), var.data_ptr(), zx, S, hf._best.data_ptr(), 1.0, None,
                           scores.data_ptr())
    assert rc == 0, rc


def columns_only():
    ext._check(lib.bbh_posterior_columns_sm(ext._h, Xd.data_ptr(), N, Xd.stride(0), tmat.data_ptr()), "bbh_posterior_columns_sm")


held = []


def unfused_only():
    held[:] = [hu._score_unfused(Xd, var, None, scores)]  # (the chunk buffer lives until the pass has been timed)


variants = {
    "a_fused_pass": fused_only,
    "b_columns_sm_store": columns_only,
    "c_unfused_pass": unfused_only,
    "a_fused_score_with_variance": lambda: hf.score(Xd, sync=False),
    "c_unfused_score_with_variance": lambda: hu.score(Xd, sync=False),
    "variance_pass": lambda: ext.posterior(Xd, out=(scores, var)),
    "d_qlogei_step": lambda: g.score_qlogei(Xd, z1, best_f, want_posterior=False),
}
for fn in variants.values():  # warm-up: code objects, workspaces, allocator blocks
    fn()
    fn()
torch.cuda.synchronize()
assert hf.last_form == "fused" and hu.last_form == "unfused"
dev = float((hf.score(Xd) - hu.score(Xd)).abs().max())
times = {k: [] for k in variants}
for _ in range(args.reps):
    for k, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1))
med = {k: statistics.median(v) for k, v in times.items()}
out = {
    "shape": {"rows": N, "d": d, "n_train": len(Xt), "baseline_rows_after_pruning": int(len(hf._pruned)), "n_extended": int(ext.n), "S": S},
    "reps": args.reps,
    "median_ms": med,
    "min_ms": {k: min(v) for k, v in times.items()},
    "max_ms": {k: max(v) for k, v in times.items()},
    "fused_over_columns_store": med["a_fused_pass"] / med["b_columns_sm_store"],
    "unfused_over_fused_pass": med["c_unfused_pass"] / med["a_fused_pass"],
    "unfused_over_fused_score": med["c_unfused_score_with_variance"] / med["a_fused_score_with_variance"],
    "fused_vs_unfused_max_abs_score_difference": dev,
    "sample_matrix_bytes_not_written": 8 * S * N,
}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "nei_pass.json").write_text(text + "\n")
