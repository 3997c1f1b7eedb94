"""Timing of the k-medoids path (csrc/bbh_pam.hip through baybe_amd.clustering) -> profiles/pam_pass.json (--out DIR: a copy there
too).

Shapes: 1e5 x 20 and 1e6 x 20 standard-normal points, k = 10.  Per shape, one child process under its own time limit runs, after an
untimed clustering of a small matrix of the same width (code objects, allocator blocks):

  upload      host -> device copy of the [N, d] matrix, and bbh_fps_prepare (the transposed matrix the kernels read)
  setup       the k-medoids++ set-up: 1 + (k - 1) calls of bbh_pam_dist_rows with the rows read back, cumsum / searchsorted on the host
  and for each of the first ``--iters`` iterations
  assign      bbh_pam_assign
  group       the stable sort by label, the clusters' column ranges and tile prefix sums, the gather of the grouped matrix (torch)
  cost        bbh_pam_cost: sum_c n_c^2 pairs x (3 d fp64 vector operations + a square root)
  update      bbh_pam_update and the read-back of medoids and flags

each timed by the host clock around work that ends in a synchronisation (the product path enqueues an iteration back to back and
synchronises once; the extra synchronisations here are what makes the parts visible).  The parent starts the children one after the
other and stops at the first that fails; nothing is retried.  ``cost_fraction_of_vector_rate`` compares the lane-operation rate of
the cost pass (3 d operations per pair; the square root is not counted) with the nominal 3.93e13 fp64 vector operations per second
of the device (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).
Usage: python scripts/gpu_pam_pass.py [--shapes 100000x20,1000000x20] [--k 10] [--iters 3] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

NOMINAL_VECTOR_OPS = 256 * 4 * 16 * 2.4e9

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100000x20,1000000x20")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--limit", type=int, default=300, help="time limit of one shape, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of pam_pass.json")
ap.add_argument("--child", default=None, help="run one shape NxD and print its times as one JSON line")
args = ap.parse_args()


def one_shape(N, d, k, iters):
    import numpy as np
    import torch

    from baybe_amd import clustering

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    rng = np.random.default_rng(0)
    clustering.k_medoids(rng.standard_normal((4096, d)), k, max_iter=2, random_state=0)

    X = rng.standard_normal((N, d))
    ms = {}
    dev, ms["upload"] = timed(lambda: clustering.DeviceRows(X, np.zeros(d), np.ones(d)))
    gp, P = dev.gp, dev.P
    medoids, ms["setup"] = timed(lambda: clustering._kpp_init(dev, k, np.random.RandomState(0)))
    med = dev._index(medoids)
    zero = torch.zeros(1, dtype=torch.int64, device=P.device)
    per_iter, pairs = [], []
    for _ in range(iters):
        it = {}
        (labels, _), it["assign"] = timed(lambda: gp.pam_assign(P, N, med))

        def group():
            grouped, perm = torch.sort(labels, stable=True)
            starts = torch.searchsorted(grouped, torch.arange(k + 1, dtype=torch.int32, device=labels.device))
            counts = starts[1:] - starts[:-1]
            tile_starts = torch.cat([zero, torch.cumsum((counts + 255) // 256, 0)])
            return perm, counts, starts, tile_starts, P.index_select(1, perm)

        (perm, counts, starts, tile_starts, Ps), it["group"] = timed(group)
        cost, it["cost"] = timed(lambda: gp.pam_cost(Ps, N, starts, tile_starts, k))
        flags, it["update"] = timed(lambda: gp.pam_update(cost, perm, N, starts, med).cpu().numpy())
        pairs.append(float((counts.double() ** 2).sum().item()))
        it["changed"] = int((flags == 2).sum())
        per_iter.append(it)
    lane_ops = pairs[-1] * 3 * d
    out = {"rows": N, "d": d, "k": k, "ms": ms, "iterations": per_iter, "pairs": pairs, "medoids": med.cpu().tolist(),
           "iteration_ms": sum(v for key, v in per_iter[-1].items() if key != "changed"),
           "cost_fraction_of_vector_rate": lane_ops / (per_iter[-1]["cost"] * 1e-3) / NOMINAL_VECTOR_OPS}
    print("TIMES " + json.dumps(out), flush=True)


if args.child:
    n, d = args.child.split("x")
    one_shape(int(n), int(d), args.k, args.iters)
    sys.exit(0)

shapes, stopped = [], None
for shape in args.shapes.split(","):
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", shape, "--k", str(args.k), "--iters", str(args.iters)],
                           capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        stopped = f"{shape}: time limit of {args.limit} s"
        break
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")]
    if r.returncode != 0 or not line:
        stopped = f"{shape}: exit status {r.returncode}: {r.stderr[-400:]}"
        break  # nothing more is started on the device after a failure
    shapes.append(json.loads(line[0][6:]))
if not shapes:
    sys.exit(f"no shape finished: {stopped}")
text = json.dumps({"nominal_fp64_vector_ops_per_s": NOMINAL_VECTOR_OPS, "stopped": stopped, "shapes": shapes}, indent=1)
print(text)
for out_dir in [ROOT / "profiles"] + ([Path(args.out)] if args.out else []):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "pam_pass.json").write_text(text + "\n")
if stopped:
    sys.exit(stopped)
