"""Timing of the farthest-point-sampling path (csrc/bbh_fps.hip through baybe_amd.sampling) -> profiles/fps_pass.json
(--out DIR: a copy there too).

Shapes: 1e5 x 15 and 1e6 x 20 standard-normal points.  Per shape, one child process under its own time limit runs, after an untimed
pass over a small matrix of the same width (code objects, allocator blocks):

  upload      host -> device copy of the [N, d] matrix
  scale       bbh_fps_prepare without an order (the scaled, transposed matrix the ranking reads)
  ranking     d stable sorts on the device (np.lexsort order)
  gather      bbh_fps_prepare with the order (the resident matrix)
  all_pairs   bbh_fps_farthest_pair: N^2 / 2 pairs x 3 d fp64 vector operations
  picks10_farthest   10 deterministic picks behind the pair, one synchronisation
  picks10_random     a "random" start and 10 picks with random tie-breaks, one synchronisation per pick

each timed by the host clock around work that ends in a synchronisation.  The parent starts the children one after the other and
stops at the first that fails; nothing is retried.  ``all_pairs_fraction_of_vector_rate`` compares the lane-operation rate of the
all-pairs pass with the nominal 3.93e13 fp64 vector operations per second of the device (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).
Usage: python scripts/gpu_fps_pass.py [--shapes 100000x15,1000000x20] [--limit SECONDS] [--out DIR]"""
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
ap.add_argument("--shapes", default="100000x15,1000000x20")
ap.add_argument("--limit", type=int, default=300, help="time limit of one shape, seconds")
ap.add_argument("--out", default=None, help="directory that receives a second copy of fps_pass.json")
ap.add_argument("--child", default=None, help="run one shape NxD and print its times as one JSON line")
args = ap.parse_args()


def one_shape(N, d):
    import numpy as np
    import torch

    from baybe_amd import sampling
    from baybe_amd.engine import HipGP

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    rng = np.random.default_rng(0)
    warm = rng.standard_normal((4096, d))
    np.random.seed(0)
    sampling.farthest_point_sampling(warm, 12, "farthest", False)
    sampling.farthest_point_sampling(warm, 12, "random", True)

    X = rng.standard_normal((N, d))
    mean, scale = sampling.standard_scaling(X)
    gp = HipGP(0)
    ms = {}
    Xd, ms["upload"] = timed(lambda: torch.from_numpy(X).to(gp._dev()))
    unranked, ms["scale"] = timed(lambda: gp.fps_prepare(Xd, mean, scale))

    def rank():
        order = torch.arange(N, device=Xd.device)
        for k in range(d):
            order = order[torch.sort(unranked[k, :N][order] + 0.0, stable=True).indices]
        return order

    order, ms["ranking"] = timed(rank)
    P, ms["gather"] = timed(lambda: gp.fps_prepare(Xd, mean, scale, order))
    (v, a, b), ms["all_pairs"] = timed(lambda: gp.fps_farthest_pair(P, N))

    def picks_farthest():
        gp.fps_greedy(P, N, starts=[a, b])
        return gp.fps_greedy(P, N, n_picks=10)

    (ranks, d2, _), ms["picks10_farthest"] = timed(picks_farthest)

    def picks_random():
        count = gp.fps_greedy(P, N, starts=[int(np.random.randint(0, N))], want_count=True)[2]
        for p in range(10):
            _, _, count = gp.fps_greedy(P, N, n_picks=1, k=int(np.random.choice(count)), want_count=p < 9)

    _, ms["picks10_random"] = timed(picks_random)
    gp.close()
    lane_ops = 0.5 * N * N * 3 * d
    out = {"rows": N, "d": d, "ms": ms, "farthest_pair": [float(v), int(a), int(b)], "first_picks": ranks.tolist()[:3],
           "all_pairs_lane_ops": lane_ops,
           "all_pairs_fraction_of_vector_rate": lane_ops / (ms["all_pairs"] * 1e-3) / NOMINAL_VECTOR_OPS,
           "pick_ms": ms["picks10_farthest"] / 10,
           "pick_matrix_bytes_per_s": 10 * N * d * 8 / (ms["picks10_farthest"] * 1e-3)}
    print("TIMES " + json.dumps(out), flush=True)


if args.child:
    n, d = args.child.split("x")
    one_shape(int(n), int(d))
    sys.exit(0)

shapes, stopped = [], None
for shape in args.shapes.split(","):
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", shape], capture_output=True, text=True,
                           timeout=args.limit)
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
    (out_dir / "fps_pass.json").write_text(text + "\n")
if stopped:
    sys.exit(stopped)
