"""Timing of one qLogNParEGO scoring pass (``HipNParEGO.score``: m variance passes over all rows, then per chunk m
``bbh_posterior_columns_sm`` launches on the targets' streams + one ``bbh_nparego_q1``) as a function of the chunk size, at
1e5 candidates x 3 targets and 1e6 candidates x 2 targets (d = 20, n = 512 training points, S = 512 base samples, pruned baseline)
-> profiles/nparego_pass.json (--out DIR: a copy there too).

Hypothesis under test: chunks whose m [S, chunk] buffers together stay well under the 256 MiB Infinity Cache let the scoring kernel
read them on-die, while small chunks pay the columns kernel's launch tail.  Per shape, after a warm-up of every variant, REPS
repetitions in which the variants alternate; a pass is timed by the host clock between two device synchronisations (its work runs on
m streams).  The same problem's qLogNEHVI pass (``HipNEHVI.score``, unchunked, same S) is recorded for orientation.
Usage: python scripts/gpu_nparego_pass.py [--reps K] [--out DIR] [--small]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from baybe_amd import engine, gp_spec, nparego  # noqa: E402
from baybe_amd.nehvi import HipNEHVI, compute_ref_point  # noqa: E402
from baybe_amd.nparego import HipNParEGO  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out", default=None, help="directory that receives a second copy of nparego_pass.json")
ap.add_argument("--small", action="store_true", help="1/50 of the rows (a rehearsal of the script, not a measurement)")
args = ap.parse_args()
d, n, S = 20, 512, 512
CHUNK_MIB = (12, 24, 48, 96, 192, 384, 768)
SHAPES = ((100_000, 3), (1_000_000, 2))
centres = (0.25, 0.75, 0.5)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


results = []
for N, m in SHAPES:
    if args.small:
        N //= 50
    rng = np.random.default_rng(0)
    X = rng.integers(0, 11, size=(N, d)) / 10.0
    Xt = rng.integers(0, 11, size=(n, d)) / 10.0
    Xt = Xt[np.sort(np.unique(Xt, axis=0, return_index=True)[1])]
    Y = np.stack([-((Xt - c) ** 2).sum(1) + 0.05 * rng.standard_normal(len(Xt)) for c in centres[:m]], axis=1)
    engines = []
    for o in range(m):
        g = engine.HipGP(0)
        g.set_model(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, Y[:, o])
        g.factorize(gp_spec.GPParams(np.full(d, 1.5), 0.02, 0.0))  # (fixed hyper-parameters: the passes are timed, not the fit)
        engines.append(g)
    Xd = torch.from_numpy(X).cuda()
    signs = np.ones(m)
    hv = HipNParEGO(engines, signs, Xt, np.full(m, 1.0 / m), n_mc_samples=S, prune_baseline=True)
    hv.prepare(7, prune_seed=8)
    log = HipNEHVI(engines, signs, Xt, compute_ref_point(Y), n_mc_samples=S, prune_baseline=True)
    log.prepare(7, prune_seed=8)

    def parego(mib):
        def run():
            nparego.CHUNK_BYTES = mib << 20
            hv.score(Xd, sync=False)
        return run

    variants = {f"nparego_chunk_{mib}MiB": parego(mib) for mib in CHUNK_MIB}
    variants["qlognehvi_unchunked"] = lambda: log.score(Xd, sync=False)
    default_bytes = nparego.CHUNK_BYTES
    scores = {}
    for k, fn in variants.items():  # warm-up: code objects, workspaces, allocator blocks
        fn()
        fn()
        torch.cuda.synchronize()
        if k.startswith("nparego"):
            scores[k] = hv.score(Xd).cpu().numpy()
    first = next(iter(scores.values()))
    assert all(np.array_equal(first, s) for s in scores.values()), "a chunk size changed a score"
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    nparego.CHUNK_BYTES = default_bytes
    med = {k: statistics.median(v) for k, v in times.items()}
    best = min((k for k in med if k.startswith("nparego")), key=med.get)
    results.append({
        "shape": {"rows": N, "targets": m, "d": d, "n_train": len(Xt), "S": S,
                  "nparego_baseline_rows_after_pruning": int(len(hv._pruned)), "qlognehvi_baseline_rows_after_pruning": int(len(log._pruned)),
                  "qlognehvi_cells": int(log.n_cells)},
        "chunk_rows": {f"nparego_chunk_{mib}MiB": int(max(1, min(N, (mib << 20) // (8 * S * m)))) for mib in CHUNK_MIB},
        "reps": args.reps,
        "median_ms": med,
        "min_ms": {k: min(v) for k, v in times.items()},
        "max_ms": {k: max(v) for k, v in times.items()},
        "best_nparego_variant": best,
        "scores_identical_across_chunk_sizes": True,
        "conditional_mean_bytes_per_pass": 8 * S * N * m,
    })
    for o in hv.outputs + log.outputs:
        o.ext.close()
    for g in engines:
        g.close()
    del Xd, hv, log
    torch.cuda.empty_cache()

out = {"default_chunk_bytes": nparego.CHUNK_BYTES, "rehearsal_only": bool(args.small), "passes": results}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "nparego_pass.json").write_text(text + "\n")
