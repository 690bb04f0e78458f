"""The Voronoi analysis (alignn_amd.voronoi) timed on a synthetic trajectory, so no model is needed: --structs B structures of
--atoms atoms (a multiple of 4) on an fcc lattice (a = 4 A) with two species, --frames frames with a Gaussian jitter of --sigma A
about the sites, a fresh one per frame, and --rcut chosen so that every cell certifies (the call is ``strict``: it would raise).

``voronoi`` without and with ``faces=True``: the median of --repeats calls timed with device events after a warm-up, and the
cells (frame x atom) and clips (cell x entries x (entries - 1) half-space clips of a polygon) per second.  Beside it, where
scipy is installed, ``scipy.spatial.Voronoi`` on the host on the 27-image point set of --scipy-frames frames of one structure,
scaled to all frames of all structures, and the largest difference of the atomic volumes between the two.  Writes one JSON file
(default profiles/voronoi_time.json) and prints it.  All in one process."""
import argparse, itertools, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import cna, voronoi

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=16)
ap.add_argument("--atoms", type=int, default=200)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--sigma", type=float, default=0.15)
ap.add_argument("--rcut", type=float, default=5.2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--scipy-frames", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voronoi_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("voronoi_time: no GPU; nothing is measured without one")
dev = "cuda"
B, n, F = args.structs, args.atoms, args.frames
if n % 4:
    sys.exit("voronoi_time: --atoms must be a multiple of 4 (fcc cells)")
cells_needed = n // 4
shape = min(((x, y, cells_needed // (x * y)) for x in range(1, cells_needed + 1) for y in range(x, cells_needed + 1)
             if cells_needed % (x * y) == 0 and cells_needed // (x * y) >= y), key=lambda s: s[2] - s[0])  # the most cubic box of fcc cells
a0 = 4.0
basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
sites = np.array([(np.array(o) + b) * a0 for o in itertools.product(*[range(s) for s in shape]) for b in basis])
cell = np.diag([s * a0 for s in shape])
rng = np.random.default_rng(11)
pos_h = np.tile(sites, (B, 1))[None] + rng.normal(0.0, args.sigma, (F, B * n, 3))
species_h = [np.where(np.arange(n) % 2 == 0, 29, 40) for _ in range(B)]
pos = torch.tensor(pos_h, device=dev)
cells = torch.tensor(np.tile(cell[None], (B, 1, 1)), device=dev)
ns = [n] * B


def timed(fn, repeats=args.repeats):
    """Median (and all) of ``repeats`` calls in ms by device events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), [round(m, 3) for m in ms]


lines = []
res = voronoi(pos, cells, ns, species_h, r_cut=args.rcut)
entries = cna(pos, cells, ns, species_h, r_cut=args.rcut).n_neighbors.double()
n_cells = F * B * n
clips = float((entries * (entries - 1.0)).sum().item())
for faces in (False, True):
    ms, runs = timed(lambda: voronoi(pos, cells, ns, species_h, r_cut=args.rcut, faces=faces))
    lines.append({"what": f"voronoi(faces={faces}) (cells + means + the read-back of the status word and of the certificate)", "ms": round(ms, 3),
                  "ms_runs": runs, "cells": n_cells, "cells_per_s": round(n_cells / (ms * 1e-3), 1), "clips_per_s": round(clips / (ms * 1e-3), 1)})
ms, runs = timed(lambda: cna(pos, cells, ns, species_h, r_cut=args.rcut))
lines.append({"what": "cna on the same lists, for orientation (at this r_cut every atom is OTHER)", "ms": round(ms, 3), "ms_runs": runs})
facts = {"entries_mean": round(float(entries.mean().item()), 2), "entries_max": int(entries.max().item()),
         "faces_mean": round(float(res.n_faces.double().mean().item()), 3), "r_max_largest": float(res.r_max.max().item()),
         "r_cut_half": args.rcut / 2.0, "complete": bool(res.complete.all().item()),
         "largest_error_of_a_frames_volume": float((res.volume.view(F, B, n).sum(-1) - float(np.linalg.det(cell))).abs().max().item())}
try:
    from scipy.spatial import ConvexHull, Voronoi
except ImportError:
    Voronoi = None
if Voronoi is not None:
    shifts = np.array(sorted(itertools.product((-1, 0, 1), repeat=3), key=lambda s: s != (0, 0, 0)), dtype=np.float64) @ cell
    k, worst, t0 = min(args.scipy_frames, F), 0.0, time.perf_counter()
    for f in range(k):
        v = Voronoi((pos_h[f, :n][None] + shifts[:, None]).reshape(-1, 3))
        volume = np.array([ConvexHull(v.vertices[v.regions[v.point_region[i]]]).volume for i in range(n)])
        worst = max(worst, float(np.abs(volume - res.volume[f, :n].cpu().numpy()).max()))
    seconds = time.perf_counter() - t0
    lines.append({"what": f"scipy.spatial.Voronoi + ConvexHull on the host, 27 images ({k} frames of one structure timed, scaled to {F} x {B})",
                  "ms": round(seconds / k * F * B * 1e3, 1), "ms_per_frame_and_structure": round(seconds / k * 1e3, 3),
                  "largest_difference_of_a_volume": worst})

out = {"tool": "tools/voronoi_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "species": 2, "frames": F, "fcc_cells": list(shape), "a": a0, "sigma": args.sigma, "r_cut": args.rcut,
                    **facts}, "runs": lines}
for line in lines:
    print(json.dumps(line), flush=True)
print(json.dumps(facts), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
