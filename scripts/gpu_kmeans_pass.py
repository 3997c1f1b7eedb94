"""Timing of the k-means path (csrc/bbh_kmeans.hip through baybe_amd.clustering) -> profiles/kmeans_pass.json (--out DIR: a copy
there too).

One shape, one process: N x d standard-normal points (default 1e5 x 15), k = 10, the reference's 50 restarts and max_iter = 1000.
After an untimed clustering of a small matrix of the same width (code objects, allocator blocks), each step under its own time
limit (a watchdog thread ends the process if a step overruns, so nothing more is started on the device after a hang):

  upload      host -> device copy of the [N, d] matrix, and bbh_fps_prepare (the transposed matrix the kernels read)
  seed        k-means++ for all 50 restarts (bbh_kmeans_seed: 4 launches per centre) and the read-back of the 50 x k positions
  iterations  the first ``--iters`` Lloyd iterations with all 50 restarts running: bbh_kmeans_pass (a pass and its finish per
              restart tile) and the read-back of shifts and flags, each timed by the host clock around that synchronisation
  fit         ``_kmeans_fit`` as a whole (draws, seeding, every iteration until the last restart stops, final labels, restart choice)
  recommend   ``HipKMeansClusteringRecommender().recommend(k, space)`` on a table-defined search space of these points: first call
              (content key, scaling, upload) and second call (resident matrix)
  sklearn     ``sklearn.cluster.KMeans(n_clusters=k, n_init=50, max_iter=1000).fit`` on the same points with the threads the
              environment grants (reported), for scale: no ratio is a pass condition

``reads_per_point_per_iteration`` is the claim the design makes: ceil(restarts / restarts_per_tile), not ``restarts``.
Usage: python scripts/gpu_kmeans_pass.py [--shape 100000x15] [--k 10] [--n-init 50] [--iters 5] [--limit SECONDS] [--no-sklearn] [--out DIR]"""
import argparse
import faulthandler
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="100000x15")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--n-init", type=int, default=50)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="time limit of one step, seconds")
ap.add_argument("--no-sklearn", action="store_true")
ap.add_argument("--out", default=None, help="directory that receives a second copy of kmeans_pass.json")
args = ap.parse_args()

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from baybe_amd import clustering  # noqa: E402

N, d = (int(v) for v in args.shape.split("x"))
k, R = args.k, args.n_init
ms = {}


def step(name, fn, limit=None):
    """``fn()`` between two synchronisations, under the step's time limit."""
    faulthandler.dump_traceback_later(limit or args.limit, exit=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms[name] = (time.perf_counter() - t0) * 1e3
    faulthandler.cancel_dump_traceback_later()
    print(f"{name}: {ms[name]:.2f} ms", flush=True)
    return out


class _Discrete:
    """The part of a discrete subspace the recommender reads: a table of points."""

    def __init__(self, frame):
        self.exp_rep = self.comp_rep = frame

    def get_candidates(self):
        return self.exp_rep, self.comp_rep


class _Space:
    def __init__(self, frame):
        self.discrete = _Discrete(frame)


rng = np.random.default_rng(0)
step("warmup", lambda: clustering.k_means(rng.standard_normal((4096, d)), k, n_init=R, max_iter=3, random_state=0))
X = rng.standard_normal((N, d))
dev = step("upload", lambda: clustering.DeviceRows(X, np.zeros(d), np.ones(d)))
rt, chunks = dev.gp.kmeans_plan(d, k, R)
T = 2 + int(np.log(k))
U = np.random.RandomState(0).random_sample((R, 1 + (k - 1) * T))
first = np.minimum((U[:, 0] * N).astype(np.int64), N - 1)
idx = step("seed", lambda: dev.kmeans_seed(first, U[:, 1:], k))
dev.kmeans_begin(idx)
iters = []
for i in range(args.iters):
    step("iteration", lambda: dev.kmeans_step(list(range(R))))
    iters.append(ms.pop("iteration"))
fit = step("fit", lambda: clustering._kmeans_fit(dev, k, n_init=R, max_iter=1000, random_state=0), limit=4 * args.limit)
space = _Space(pd.DataFrame(X, columns=[f"x{i}" for i in range(d)]))
rec = clustering.HipKMeansClusteringRecommender()
np.random.seed(0)
picked = step("recommend_first", lambda: rec.recommend(k, space), limit=4 * args.limit)
np.random.seed(0)
again = step("recommend_resident", lambda: rec.recommend(k, space), limit=4 * args.limit)
assert picked.index.tolist() == again.index.tolist()
out = {"rows": N, "d": d, "k": k, "n_init": R, "restarts_per_tile": rt, "chunks": chunks,
       "reads_per_point_per_iteration": -(-R // rt), "ms": ms, "iteration_ms": iters, "fit_n_iter_of_winner": fit[3],
       "fit_inertia": fit[2], "selection": picked.index.tolist()}
if not args.no_sklearn:
    from sklearn.cluster import KMeans

    np.random.seed(0)
    t0 = time.perf_counter()
    faulthandler.dump_traceback_later(10 * args.limit, exit=True)
    model = KMeans(n_clusters=k, n_init=R, max_iter=1000).fit(X)
    faulthandler.cancel_dump_traceback_later()
    out["sklearn"] = {"fit_ms": (time.perf_counter() - t0) * 1e3, "inertia": float(model.inertia_), "n_iter_of_winner": int(model.n_iter_),
                      "threads": os.environ.get("OMP_NUM_THREADS", "unset")}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "kmeans_pass.json").write_text(text + "\n")
