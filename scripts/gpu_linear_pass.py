"""Timing of the Bayesian linear surrogate's moment pass (csrc/bbh_linear.hip through baybe_amd.linear) -> profiles/linear_pass.json
(--out DIR: a copy there too).

Shapes in one process (default 100000x15 and 1000000x20 with every column kept, 100000x300 with 161 kept columns, 100000x40 with
32 kept columns - the largest model the register form takes - and, for the crossover of form "auto", 1000000x16 with 16 and 1000000x40
with 32 kept columns; every model of at most 32 kept columns is timed in both forms, so that the crossover can be moved).  The model of
a shape is synthetic (a random symmetric PSD ``sigma_``, random kept columns): the pass does not care where its tables come from, and
an ARD fit that keeps exactly k columns cannot be ordered.  Per shape, after an untimed pass over a small matrix of the same width,
each step under its own time limit (a watchdog ends the process if a step overruns, so nothing more is started on the device after a
hang).  A device step is timed in windows of about ``--window-ms``: as many back-to-back calls as that takes between two
synchronisations, ``--reps`` windows, time per call = window / calls; the median is reported next to every window.  A call includes
the read-back of the column list that ``bbh_linear_moments`` checks before it launches.

  upload        host -> device copy of the [N, d] candidate matrix (once per search space: the recommender keeps it resident)
  register      ``bbh_linear_moments`` in the register form (k <= 32)
  block         ``bbh_linear_moments`` in the block form (any k)
  sklearn       ``ARDRegression.predict(X~, return_std=True)`` on the same rows on the host, on the threads the environment grants, with
                the scaling of the rows timed separately - a reported baseline, not a target; the deviation of the device's moments
                from it is recorded

The record also holds what a pass must move at the least (N d 8 bytes of candidates, 16 N bytes of results) and its multiply-adds
(N (k (k + 1) / 2 + k)), so a rate can be read off; no share of peak is claimed.

Usage: python scripts/gpu_linear_pass.py [--shapes 100000x15:15,1000000x20:20,100000x300:161,100000x40:32,1000000x16:16,1000000x40:32] [--reps 10] [--window-ms 100]
                                         [--limit SECONDS] [--out DIR]"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100000x15:15,1000000x20:20,100000x300:161,100000x40:32,1000000x16:16,1000000x40:32")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--window-ms", type=float, default=100.0, help="least duration of one timed window")
ap.add_argument("--limit", type=int, default=120, help="time limit of one step, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of linear_pass.json")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.linear_model import ARDRegression  # noqa: E402

from baybe_amd import linear as L  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("gpu_linear_pass.py measures on the device: no HIP device here")


def timed(fn, limit=None, sync=True):
    """Milliseconds of ``fn()`` (between two synchronisations), under the step's time limit; and its result."""
    faulthandler.dump_traceback_later(limit or args.limit, exit=True)
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    faulthandler.cancel_dump_traceback_later()
    return ms, out


def repeated(name, fn, rec):
    """``--reps`` timed windows of ``calls`` back-to-back calls each, one synchronisation before and one after a window; ``calls`` is
    chosen from one trial call so that a window lasts about ``--window-ms``.  Reported per call: window time / calls."""
    trial = timed(fn)[0]
    calls = int(min(2000, max(1, -(-args.window_ms // max(trial, 1e-3)))))

    def window():
        for _ in range(calls):
            fn()

    runs = [timed(window)[0] / calls for _ in range(args.reps)]
    rec[name] = {"median_ms": statistics.median(runs), "calls_per_window": calls, "runs_ms": runs}
    print(f"  {name}: median {rec[name]['median_ms']:.4f} ms per call ({calls} calls per window) of {[round(r, 4) for r in runs]}", flush=True)


def synthetic_model(d, k, rng):
    """(what ``pack_linear`` reads, lo, hi): k of d columns kept, ``sigma_`` symmetric PSD of half rank."""
    kept = np.sort(rng.permutation(d)[:k])
    lam = np.full(d, 1e6)
    lam[kept] = 0.5 + rng.random(k)
    coef = np.zeros(d)
    coef[kept] = rng.standard_normal(k)
    A = rng.standard_normal((k, (k + 1) // 2))
    lo = rng.integers(-4, 5, d).astype(np.float64)
    hi = lo + rng.integers(1, 5, d).astype(np.float64)
    return SimpleNamespace(lambda_=lam, threshold_lambda=1e4, coef_=coef, intercept_=0.375, sigma_=A @ A.T / k, alpha_=7.0), lo, hi


def sklearn_twin(model, d):
    """An ``ARDRegression`` whose ``predict`` reads the synthetic model's arrays."""
    ard = ARDRegression(max_iter=1).fit(np.eye(d + 1, d), np.arange(d + 1.0))
    for key in ("lambda_", "threshold_lambda", "coef_", "intercept_", "sigma_", "alpha_"):
        setattr(ard, key, getattr(model, key))
    ard.X_offset_ = np.zeros(d)  # (1.7.2 does not read it in predict; kept consistent all the same)
    return ard


def one_shape(N, d, k):
    rec = {"rows": N, "d": d, "kept": k}
    print(f"{N} x {d}, {k} kept columns", flush=True)
    rng = np.random.default_rng(0)
    model, lo, hi = synthetic_model(d, k, rng)
    packed = L.pack_linear(model, lo, hi)
    eng = L.HipLinearEngine(0)
    rec["upload_model_ms"], _ = timed(lambda: eng.set_linear(packed, d, -1.5, 2.5))
    X = lo + (hi - lo) * rng.random((N, d))
    small = eng._as_dev(X[:4096])
    rec["upload_candidates_ms"], Xd = timed(lambda: eng._as_dev(X))
    forms = (["register"] if k <= L.REGISTER_MAX_KEPT else []) + ["block"]
    results = {}
    for form in forms:
        timed(lambda: eng.posterior(small, form=form))  # warm-up, untimed
        timed(lambda: eng.posterior(Xd, form=form))
        repeated(form, lambda: eng.posterior(Xd, form=form), rec)
        assert eng.linear_last_form() == form
        rec[form]["rows_per_s"] = N / (rec[form]["median_ms"] * 1e-3)
        results[form] = tuple(t.cpu().numpy() for t in eng.posterior(Xd, form=form))
    rec["candidate_bytes"], rec["result_bytes"] = N * d * 8, N * 16
    rec["multiply_adds"] = N * (k * (k + 1) // 2 + k)
    ard = sklearn_twin(model, d)
    ms_scale, Xs = timed(lambda: (X - lo) / (hi - lo), 10 * args.limit, sync=False)
    ms_pred, (mean, std) = timed(lambda: ard.predict(Xs, return_std=True), 10 * args.limit, sync=False)
    want_mean, want_var = -1.5 + 2.5 * mean, 2.5 * 2.5 * std**2
    rec["sklearn"] = {"scale_ms": ms_scale, "predict_return_std_ms": ms_pred, "rows_per_s": N / ((ms_scale + ms_pred) * 1e-3),
                      "threads": os.environ.get("OMP_NUM_THREADS", "unset"),
                      "max_abs_deviation_mean": {f: float(np.abs(results[f][0] - want_mean).max()) for f in forms},
                      "max_abs_deviation_var": {f: float(np.abs(results[f][1] - want_var).max()) for f in forms}}
    print(f"  sklearn on the host: scaling {ms_scale:.1f} ms + predict(return_std=True) {ms_pred:.1f} ms; device vs sklearn "
          f"{rec['sklearn']['max_abs_deviation_mean']} / {rec['sklearn']['max_abs_deviation_var']}", flush=True)
    eng.close()
    return rec


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window_ms": args.window_ms, "shapes": []}
for spec in args.shapes.split(","):
    shape, k = spec.split(":")
    N, d = (int(v) for v in shape.split("x"))
    out["shapes"].append(one_shape(N, d, int(k)))
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "linear_pass.json").write_text(text + "\n")
