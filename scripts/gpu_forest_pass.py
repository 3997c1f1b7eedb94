"""Timing of the random forest path (csrc/bbh_forest.hip through baybe_amd.forest) -> profiles/forest_pass.json (--out DIR: a copy
there too).

Two shapes in one process (default 100000x15 with a forest fitted on n = 256 rows, 1000000x20 with n = 512; 100 fully grown trees
each, uniform rows, a smooth response plus noise).  Per shape, after an untimed pass over a small matrix of the same width (code
objects, allocator blocks), each step under its own time limit (a watchdog ends the process if a step overruns, so nothing more is
started on the device after a hang).  A device step is timed in windows of about ``--window-ms``: as many back-to-back calls as
that takes between two synchronisations (a single call of 0.5 ms would measure the synchronisation and the launch as much as the
kernel), ``--reps`` windows, time per call = window / calls; the median is reported next to every window:

  fit_host      ``RandomForestRegressor(n_estimators=100, random_state=0).fit`` - scikit-learn on the host, the floor of a forest
                ``recommend()`` here as in the reference; then ``pack_forest`` and the upload of the node tables
  upload        host -> device copy of the [N, d] candidate matrix (once per search space: the recommender keeps it resident)
  moments       ``bbh_forest_moments``: mean and unbiased variance over the trees (two traversals of every tree)
  qlogei        ``bbh_forest_mc_acq``: the fused qLogEI pass, S = 512 samples, without and with 4 pending points
  greedy3       ``HipForestAcq.greedy`` for a batch of 3 (three fused passes, three selections, three one-row predictions)
  cpu           on ``--cpu-rows`` of the candidates (stated in the record): ``estimator.predict`` per tree as the reference calls it,
                and the numpy oracle's qLogEI scoring of the resulting [T, rows] matrix (tests/_oracle_forest.py), on the threads the
                environment grants - for scale: no ratio is a pass condition, and the rows-per-second figures are what to compare

The record also holds what the passes must move at the least (N d 8 bytes of candidates; the node tables stay in LDS / cache), so a
rate can be read off; no share of peak is claimed - the traversal is latency-bound gather-and-compare, not a streaming kernel.

Usage: python scripts/gpu_forest_pass.py [--shapes 100000x15:256,1000000x20:512] [--trees 100] [--reps 10] [--window-ms 100] [--cpu-rows 20000]
                                         [--limit SECONDS] [--out DIR]"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100000x15:256,1000000x20:512")
ap.add_argument("--trees", type=int, default=100)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--window-ms", type=float, default=100.0, help="least duration of one timed window")
ap.add_argument("--cpu-rows", type=int, default=20000)
ap.add_argument("--limit", type=int, default=120, help="time limit of one step, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of forest_pass.json")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.ensemble import RandomForestRegressor  # noqa: E402

import _oracle_forest as of  # noqa: E402
from baybe_amd import forest as F  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("gpu_forest_pass.py measures on the device: no HIP device here")
S = 512


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
    calls = int(min(500, max(1, -(-args.window_ms // max(trial, 1e-3)))))

    def window():
        for _ in range(calls):
            fn()

    runs = [timed(window)[0] / calls for _ in range(args.reps)]
    rec[name] = {"median_ms": statistics.median(runs), "calls_per_window": calls, "runs_ms": runs}
    print(f"  {name}: median {rec[name]['median_ms']:.3f} ms per call ({calls} calls per window) of {[round(r, 3) for r in runs]}", flush=True)


class _Holder:
    def __init__(self, engine):
        self.engine = engine


def one_shape(N, d, n):
    rec = {"rows": N, "d": d, "train_rows": n, "trees": args.trees, "S": S}
    print(f"{N} x {d}, forest of {args.trees} trees on {n} rows", flush=True)
    rng = np.random.default_rng(0)
    w = np.cos(np.arange(d) + 1.0)
    train_x = rng.random((n, d))
    train_y = np.sin(3.0 * train_x @ w / np.sqrt(d)) + 0.1 * rng.standard_normal(n)
    ms, model = timed(lambda: RandomForestRegressor(n_estimators=args.trees, random_state=0).fit(train_x, train_y), 10 * args.limit, sync=False)
    rec["fit_host_ms"] = ms
    rec["fit_host_threads"] = "n_jobs=None (one thread)"
    ms, packed = timed(lambda: F.pack_forest(model.estimators_), sync=False)
    rec["pack_ms"] = ms
    sizes = np.diff(packed["offsets"])
    rec["nodes_total"], rec["nodes_max_per_tree"] = int(sizes.sum()), int(sizes.max())
    eng = F.HipForestEngine(0)
    eng._X_train = train_x
    rec["lds_nodes"] = eng.forest_lds_nodes()
    rec["upload_forest_ms"], _ = timed(lambda: eng.set_forest(packed, d))
    X = rng.random((N, d))
    small = eng._as_dev(X[:4096])
    rec["upload_candidates_ms"], Xd = timed(lambda: eng._as_dev(X))
    best = eng.best_f(1.0)
    acq = F.HipForestAcq(_Holder(eng), "qLogEI", 1.0, best, S)
    acq.prepare(1234, None)
    rec["trees_read_by_a_sample"] = int((acq.counts_host > 0).sum())
    timed(lambda: (eng.forest_moments(eng.forest, small), acq.score(small)))  # warm-up, untimed
    timed(lambda: (eng.forest_moments(eng.forest, Xd), acq.score(Xd)))
    repeated("moments", lambda: eng.forest_moments(eng.forest, Xd), rec)
    repeated("qlogei_k0", lambda: acq.score(Xd), rec)
    acq.prepare(1234, X[:4])
    timed(lambda: acq.score(Xd))
    repeated("qlogei_k4", lambda: acq.score(Xd), rec)
    timed(lambda: acq.greedy(Xd, 3, seed=1234))  # (first use of the loop's small tensor ops)
    repeated("greedy3", lambda: acq.greedy(Xd, 3, seed=1234), rec)
    rec["greedy3_indices"] = acq.greedy(Xd, 3, seed=1234).indices
    rec["candidate_bytes"] = N * d * 8
    rec["qlogei_k0_rows_per_s"] = N / (rec["qlogei_k0"]["median_ms"] * 1e-3)
    rec["moments_rows_per_s"] = N / (rec["moments"]["median_ms"] * 1e-3)
    # the host's way, on a stated sample of the rows
    rows = min(args.cpu_rows, N)
    Xs = X[:rows]
    ms_pred, P = timed(lambda: np.stack([e.predict(Xs) for e in model.estimators_]), 10 * args.limit, sync=False)
    idx = F.ensemble_member_indices(S, args.trees, 1234)
    ms_score, want = timed(lambda: of.scores("qLogEI", P, None, idx, best, 1.0), 10 * args.limit, sync=False)
    acq.prepare(1234, None)
    got = acq.score(eng._as_dev(Xs)).cpu().numpy()
    rec["cpu"] = {"rows": rows, "predict_per_tree_ms": ms_pred, "oracle_qlogei_ms": ms_score,
                  "rows_per_s": rows / ((ms_pred + ms_score) * 1e-3), "threads": os.environ.get("OMP_NUM_THREADS", "unset"),
                  "max_abs_deviation_device_vs_oracle": float(np.abs(got - want).max())}
    print(f"  cpu on {rows} rows: predict {ms_pred:.1f} ms + oracle scoring {ms_score:.1f} ms; device vs oracle "
          f"{rec['cpu']['max_abs_deviation_device_vs_oracle']:.2e}", flush=True)
    eng.close()
    return rec


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window_ms": args.window_ms, "shapes": []}
for spec in args.shapes.split(","):
    shape, n = spec.split(":")
    N, d = (int(v) for v in shape.split("x"))
    out["shapes"].append(one_shape(N, d, int(n)))
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "forest_pass.json").write_text(text + "\n")
