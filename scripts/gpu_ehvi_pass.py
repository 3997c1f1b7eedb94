"""Timing of one qEHVI / qLogEHVI scoring pass (csrc/bbh_ehvi.hip) next to its yardsticks -> profiles/ehvi_pass.json (--out DIR: a
copy there too).

Shape: N = 1e5 candidates in 3 dimensions, m = 3 targets (GPs fitted on 24 rows), S = 128 base samples, p = 0, 2, 4 and 7 pending
points (rows of the candidate set), the cell list of the models' posterior means at the measurement rows.  Per p and form (qLogEHVI /
qEHVI) the kernel time is the handle's event timing of the launch (families "q1" / "pending": the scoring kernel and its finish
kernel), with the factors in LDS and in the workspace, and - the A/B of KERNELS.md 4.14 - under two settings of BBH_EHVI_SLICE:
unset (slices of 16 samples over a second grid dimension) and 0 (one thread per candidate walks all samples).

Yardsticks, same rows, same process: the qLogNEHVI scoring pass (family "nehvi": the cell kernel of bbh_qnehvi.hip after
``HipNEHVI.prepare``; its conditional-mean columns, family "columns", are reported next to it) and the m single-target posterior
passes (family "posterior").  No ratio is a requirement.

A setting of the switch is one child process (switches are read when a handle is created); the parent starts them one after the
other, each under its own time limit, and stops at the first that fails.
Usage: python scripts/gpu_ehvi_pass.py [--rows N] [--pending P ...] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--pending", type=int, nargs="+", default=[0, 2, 4, 7])
ap.add_argument("--limit", type=int, default=420, help="time limit of one child process, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of ehvi_pass.json")
ap.add_argument("--child", action="store_true", help="run the passes under the current environment and print the times as one JSON line")
args = ap.parse_args()
S, M, D, N_TRAIN = 128, 3, 3, 24


def passes():
    import numpy as np
    import torch

    from baybe_amd import engine, gp_spec
    from baybe_amd.ehvi import HipEHVI
    from baybe_amd.nehvi import HipNEHVI, compute_ref_point

    rng = np.random.default_rng(0)
    Xt = rng.random((N_TRAIN, D))
    Y = np.stack([-((Xt - 0.25) ** 2).sum(1), -((Xt - 0.75) ** 2).sum(1), -np.abs(Xt - 0.5).sum(1)], 1) + 0.05 * rng.standard_normal((N_TRAIN, M))
    engines = []
    for o in range(M):
        g = engine.HipGP(0)
        g.set_model(gp_spec.GPSpec.baybe_default(D, np.zeros(D), np.ones(D)), Xt, Y[:, o])
        g.fit()
        engines.append(g)
    signs = np.ones(M)
    ref = compute_ref_point(Y)
    X = torch.rand((args.rows, D), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    small = X[:2048].contiguous()
    times = {}

    def family_ms(engs, family, fn):
        for e in engs:
            e.timing(True, [family])
            e.timing_read(True, family)
        keep = fn()
        torch.cuda.synchronize()
        total = sum(e.timing_read(True, family)[0] for e in engs)
        for e in engs:
            e.timing(False)
        del keep
        return total

    sliced = "BBH_EHVI_SLICE" not in os.environ
    if sliced:  # the yardsticks once, in the default child
        for e in engines:
            e.posterior(small)
        times["posterior_passes"] = family_ms(engines, "posterior", lambda: [e.posterior(X) for e in engines])
        nehvi = HipNEHVI(engines, signs, Xt, ref, n_mc_samples=S, prune_baseline=True, device=0)
        nehvi.prepare(1234, prune_seed=4321)
        nehvi.score(small)
        ext = [o.ext for o in nehvi.outputs]
        times["qlognehvi_cells"] = family_ms(ext[:1], "nehvi", lambda: nehvi.score(X))
        times["qlognehvi_columns"] = family_ms(ext, "columns", lambda: nehvi.score(X))
        times["qlognehvi_cells_per_sample"] = float(nehvi.n_cells) / S
        del nehvi
    for log, name in ((True, "qLogEHVI"), (False, "qEHVI")):
        sc = HipEHVI(engines, signs, Xt, ref, log=log, n_mc_samples=S)
        cells = sc.cells()
        times["cells"] = len(cells[0])
        for p in args.pending:
            z = sc.base_samples(1 + p, 7)
            for Xs, timed in ((small, False), (X, True)):  # untimed at 2048 rows: code objects, workspaces
                Xd, mean, var = sc._moments(Xs)
                if p == 0:
                    variants = {"q1": lambda: engines[0].ehvi_acq(log, mean, var, cells, z[:, 0, :])}
                    family = "q1"
                else:
                    pend = X[5000:5000 + p].cpu().numpy()
                    cross, stats = sc._pending_terms(Xd, pend)
                    variants = {form_name: (lambda form=form: engines[0].ehvi_acq(log, mean, var, cells, z, cross=cross, stats=stats, form=form))
                                for form_name, form in (("lds", 0), ("ws", 1))}
                    family = "pending"
                for k, fn in variants.items():
                    if not timed:
                        fn()
                        torch.cuda.synchronize()
                    else:
                        times[f"{name}-p{p}-{k}"] = family_ms(engines[:1], family, fn)
                sc._clear_pending()
    for g in engines:
        g.close()
    print("TIMES " + json.dumps(times), flush=True)


if args.child:
    passes()
    sys.exit(0)

results, stopped = {}, None
for label, value in (("slice16", None), ("one_slice", "0")):
    env = dict(os.environ)
    env.pop("BBH_EHVI_SLICE", None)
    if value is not None:
        env["BBH_EHVI_SLICE"] = value
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--rows", str(args.rows), "--pending",
                            *map(str, args.pending)], capture_output=True, text=True, timeout=args.limit, env=env)
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
out = {"shape": {"rows": args.rows, "S": S, "targets": M, "pending": args.pending, "train_rows": N_TRAIN}, "stopped": stopped, "ms": results}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "ehvi_pass.json").write_text(text + "\n")
