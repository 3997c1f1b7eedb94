"""Timing of the Gaussian mixture path (csrc/bbh_gmm.hip through baybe_amd.clustering) -> profiles/gmm_pass.json (--out DIR: a copy
there too).

One shape, one process: N x d standard-normal points (default 1e5 x 20), k = 10, the reference's defaults (one restart, k-means
initialisation, tol = 1e-3, at most 100 iterations).  After an untimed fit of a small matrix of the same width (code objects,
allocator blocks), each step under its own time limit (a watchdog thread ends the process if a step overruns, so nothing more is
started on the device after a hang):

  upload      host -> device copy of the [N, d] matrix, and bbh_fps_prepare (the transposed matrix the kernels read)
  init        the k-means initialisation, the M-step from its labels and the precision factors (``_kmeans_run``, ``gmm_begin``)
  e_step      ``--iters`` E-steps from the initial parameters (bbh_gmm_estep), each between two synchronisations
  m_step      ``--iters`` M-steps from the last log_resp with their precision factors (bbh_gmm_mstep, bbh_gmm_precision)
  fit         ``_gmm_fit`` as a whole (draws, initialisation, every iteration until the restart stops, prediction)
  recommend   ``HipGaussianMixtureClusteringRecommender().recommend(k, space)`` on a table-defined search space of these points: first
              call (content key, scaling, upload) and second call (resident matrix)
  sklearn     ``sklearn.mixture.GaussianMixture(n_components=k).fit`` on the same points with the threads the environment grants
              (reported), for scale: no ratio is a pass condition

Usage: python scripts/gpu_gmm_pass.py [--shape 100000x20] [--k 10] [--n-init 1] [--iters 5] [--limit SECONDS] [--no-sklearn] [--out DIR]"""
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
ap.add_argument("--shape", default="100000x20")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--n-init", type=int, default=1)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="time limit of one step, seconds")
ap.add_argument("--no-sklearn", action="store_true")
ap.add_argument("--out", default=None, help="directory that receives a second copy of gmm_pass.json")
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


def _init(dev):
    clustering._kmeans_run(dev, k, R, 300, 1e-4, "k-means++", np.random.RandomState(0))
    return dev.gmm_begin(k, 1e-6)


rng = np.random.default_rng(0)
step("warmup", lambda: clustering.gaussian_mixture(rng.standard_normal((4096, d)), k, n_init=R, max_iter=3, random_state=0))
X = rng.standard_normal((N, d))
dev = step("upload", lambda: clustering.DeviceRows(X, np.zeros(d), np.ones(d)))
kc, tps = dev.gp.gmm_plan(d, k, N)
_, _, G = step("init", lambda: _init(dev))
rid = dev._rid(np.arange(min(R, G)))
e_steps, m_steps = [], []
for i in range(args.iters):
    step("e_step", lambda: dev.gp.gmm_estep(dev.P, dev.m, dev._gm, rid, dev._gm_lr, dev._gm_lab, 0))
    e_steps.append(ms.pop("e_step"))
for i in range(args.iters):
    step("m_step", lambda: dev.gp.gmm_mstep(dev.P, dev.m, dev._gm, rid, 1e-6, log_resp=dev._gm_lr, base=0))
    m_steps.append(ms.pop("m_step"))
fit = step("fit", lambda: clustering._gmm_fit(dev, k, n_init=R, random_state=0), limit=4 * args.limit)
space = _Space(pd.DataFrame(X, columns=[f"x{i}" for i in range(d)]))
rec = clustering.HipGaussianMixtureClusteringRecommender({"n_init": R, "random_state": 0})
np.random.seed(0)
picked = step("recommend_first", lambda: rec.recommend(k, space), limit=4 * args.limit)
np.random.seed(0)
again = step("recommend_resident", lambda: rec.recommend(k, space), limit=4 * args.limit)
assert picked.index.tolist() == again.index.tolist()
out = {"rows": N, "d": d, "k": k, "n_init": R, "components_per_chunk": kc, "tiles_per_strip": tps, "restarts_per_group": G, "ms": ms,
       "e_step_ms": e_steps, "m_step_ms": m_steps, "fit_n_iter": fit[4], "fit_lower_bound": fit[3], "fit_converged": fit[5],
       "flops_per_sweep": 2.0 * N * k * d * d, "selection": picked.index.tolist()}
if not args.no_sklearn:
    from sklearn.mixture import GaussianMixture

    t0 = time.perf_counter()
    faulthandler.dump_traceback_later(10 * args.limit, exit=True)
    model = GaussianMixture(n_components=k, n_init=R, random_state=0).fit(X)
    faulthandler.cancel_dump_traceback_later()
    out["sklearn"] = {"fit_ms": (time.perf_counter() - t0) * 1e3, "lower_bound": float(model.lower_bound_), "n_iter": int(model.n_iter_),
                      "threads": os.environ.get("OMP_NUM_THREADS", "unset")}
text = json.dumps(out, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "gmm_pass.json").write_text(text + "\n")
