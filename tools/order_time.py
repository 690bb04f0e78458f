"""Structural order analysis (alignn_amd.order) timed per function on a synthetic trajectory, so no model is needed: --structs B
structures of --atoms atoms with two species, --frames frames of N(0, 0.15 A) displacements about a simple-cubic-like lattice
(spacing 2.65 A: with 200 atoms a cell of 15.9 A, |h| <= 20 at q_max = 8); the angle distribution and q_4, q_6 with --rcut, S(q)
with --qmax.

Per function: the median of --repeats calls timed with device events after a warm-up call, and the triplets or (atom, vector)
phases per second.  Beside each, the same quantity as plain torch expressions on the same device, timed on --torch-frames frames
and scaled to all: per frame the dense distances to every image, the --torch-neighbors nearest by ``topk``, their cosine matrix,
``acos`` and ``histc`` (every triplet, no species rows) or the Legendre recurrence; and ``exp(2 pi i f . h)`` summed over the
atoms (the total S only).  The largest difference between the two is printed with each.  Writes one JSON file (default
profiles/order_time.json) and prints it.  All in one process."""
import argparse, itertools, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import adf, steinhardt, structure_factor
from tests import traj_ref

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=16)
ap.add_argument("--atoms", type=int, default=200)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--rcut", type=float, default=3.5)
ap.add_argument("--qmax", type=float, default=8.0)
ap.add_argument("--bins", type=int, default=180)
ap.add_argument("--qbins", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--torch-frames", type=int, default=20)
ap.add_argument("--torch-neighbors", type=int, default=24)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("order_time: no GPU; nothing is measured without one")
dev = "cuda"
B, n, F = args.structs, args.atoms, args.frames
rng = np.random.default_rng(7)
side = int(np.ceil(n ** (1 / 3)))
grid = np.array(list(itertools.product(range(side), repeat=3)), dtype=np.float64)[:n] * 2.65
cell = np.eye(3) * side * 2.65
pos_h = np.tile(grid, (B, 1))[None] + rng.normal(0.0, 0.15, (F, B * n, 3))
species_h = [np.where(np.arange(n) % 2 == 0, 3, 8) for _ in range(B)]
pos = torch.tensor(pos_h, device=dev)
cells = torch.tensor(np.tile(cell[None], (B, 1, 1)), device=dev)
ns = [n] * B
M = traj_ref.image_range(cell, args.rcut)
tf = min(args.torch_frames, F)


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
# --- the neighbour shells: angle distribution and Steinhardt parameters ---------------------------------------------------------------
st = steinhardt(pos, cells, ns, species_h, r_cut=args.rcut, ls=(4, 6))
nb_count = st.n_neighbors.long()
triplets = int((nb_count * (nb_count - 1) // 2).sum().item())
ms, runs = timed(lambda: adf(pos, cells, ns, species_h, r_cut=args.rcut, n_bins=args.bins))
lines.append({"what": "adf (triplet walk + finish + the status word's read-back)", "ms": round(ms, 3), "ms_runs": runs,
              "triplets": triplets, "triplets_per_s": round(triplets / (ms * 1e-3), 1), "neighbors_at_most": int(nb_count.max().item()),
              "compulsory_bytes": F * B * n * 24})
ms, runs = timed(lambda: steinhardt(pos, cells, ns, species_h, r_cut=args.rcut, ls=(4, 6)))
lines.append({"what": "steinhardt q4, q6 (triplet walk + means + the status word's read-back)", "ms": round(ms, 3), "ms_runs": runs,
              "triplets": triplets, "triplets_per_s": round(triplets / (ms * 1e-3), 1)})

shifts = torch.tensor(np.array(list(itertools.product(*[range(-m, m + 1) for m in M])), dtype=np.float64) @ cell, device=dev)
inv = torch.linalg.inv(cells)
K = args.torch_neighbors
upper = torch.triu(torch.ones(K, K, dtype=torch.bool, device=dev), 1)
own = (torch.eye(n, device=dev)[None, :, :, None] > 0) & (shifts.abs().sum(1) == 0)[None, None, None, :]


def torch_cosines(f):
    """-> (cos [B, n, K, K] of the K nearest (j, image) of every atom, which pairs are two neighbours, neighbours [B, n])."""
    x = pos[f].view(B, n, 3)
    dp = x[:, None, :, :] - x[:, :, None, :]
    df = dp @ inv[:, None]
    d0 = (df - torch.round(df)) @ cells[:, None]
    d = (d0[:, :, :, None, :] + shifts[None, None, None]).reshape(B, n, -1, 3)
    r = torch.sqrt((d * d).sum(-1))
    r = torch.where(own.reshape(1, n, -1), torch.full_like(r, 1e30), r)
    rk, at = torch.topk(r, K, dim=-1, largest=False)
    dk = torch.gather(d, 2, at[..., None].expand(-1, -1, -1, 3))
    inside = rk < args.rcut
    cos = ((dk @ dk.transpose(-1, -2)) / (rk[..., :, None] * rk[..., None, :])).clamp(-1.0, 1.0)
    return cos, inside[..., :, None] & inside[..., None, :] & upper, inside.sum(-1)


def torch_adf(frames):
    hist = torch.zeros(args.bins, dtype=torch.float64, device=dev)
    for f in range(frames):
        cos, pair, _ = torch_cosines(f)
        hist += torch.histc(torch.acos(cos[pair]), bins=args.bins, min=0.0, max=float(np.pi))
    return hist


def torch_steinhardt(frames):
    out = torch.empty(frames, B * n, 2, dtype=torch.float64, device=dev)
    for f in range(frames):
        cos, pair, nbs = torch_cosines(f)
        pm, pn, sums = torch.ones_like(cos), cos, {}
        for d in range(1, 7):
            if d in (4, 6):
                sums[d] = torch.where(pair, pn, torch.zeros_like(pn)).sum((-1, -2))
            pm, pn = pn, ((2 * d + 1) * cos * pn - d * pm) / (d + 1)
        nn = nbs.double()
        for u, d in enumerate((4, 6)):
            out[f, :, u] = torch.sqrt(((nn + 2.0 * sums[d]) / (nn * nn)).clamp_min(0.0)).reshape(-1)
    return out


assert int(nb_count.max().item()) <= K, "raise --torch-neighbors: the torch expressions would drop neighbours"
ms_t, runs_t = timed(lambda: torch_adf(tf), repeats=3)
got = adf(pos[:tf].contiguous(), cells, ns, None, r_cut=args.rcut, n_bins=args.bins).counts[:, 0, 0].sum(0)
lines.append({"what": f"adf as torch expressions (every triplet only, {tf} frames timed, scaled to {F})", "ms": round(ms_t * F / tf, 3),
              "ms_runs_of_the_timed_frames": runs_t, "triplets_per_s": round(triplets / (ms_t * F / tf * 1e-3), 1),
              "histograms_differ_in": int((got.double() - torch_adf(tf)).abs().sum().item())})  # (triplets at a bin edge may move)
ms_t, runs_t = timed(lambda: torch_steinhardt(tf), repeats=3)
lines.append({"what": f"steinhardt as torch expressions ({tf} frames timed, scaled to {F})", "ms": round(ms_t * F / tf, 3),
              "ms_runs_of_the_timed_frames": runs_t, "triplets_per_s": round(triplets / (ms_t * F / tf * 1e-3), 1),
              "largest_difference_of_q": float((st.q[:tf] - torch_steinhardt(tf)).abs().max().item())})

# --- S(q) -------------------------------------------------------------------------------------------------------------------------------
sq = structure_factor(pos, cells, ns, species_h, q_max=args.qmax, n_bins=args.qbins)
V = int(sq.hkl[0].shape[0])
phases = F * B * n * V
ms, runs = timed(lambda: structure_factor(pos, cells, ns, species_h, q_max=args.qmax, n_bins=args.qbins))
lines.append({"what": "structure_factor (vectors + accumulate + bin + the counts' read-back)", "ms": round(ms, 3), "ms_runs": runs,
              "vectors_per_structure": V, "h_at_most": int(sq.hkl[0].abs().max().item()), "phases": phases,
              "phases_per_s": round(phases / (ms * 1e-3), 1), "compulsory_bytes": F * B * n * 24})
hkl_t = sq.hkl[0].double()


def torch_sq(frames):
    total = torch.zeros(B, V, dtype=torch.float64, device=dev)
    for f in range(frames):
        fr = pos[f].view(B, n, 3) @ inv
        ph = (2.0 * np.pi) * (fr @ hkl_t.T)  # [B, n, V]
        re, im = torch.cos(ph).sum(1), torch.sin(ph).sum(1)
        total += re * re + im * im
    return total / (frames * n)


ms_t, runs_t = timed(lambda: torch_sq(tf), repeats=3)
ours = torch.stack(structure_factor(pos[:tf].contiguous(), cells, ns, None, q_max=args.qmax, n_bins=args.qbins).s_vectors)[:, 0]
ref_t = torch_sq(tf)
lines.append({"what": f"S(q) as torch expressions (the total only, {tf} frames timed, scaled to {F})", "ms": round(ms_t * F / tf, 3),
              "ms_runs_of_the_timed_frames": runs_t, "phases_per_s": round(phases / (ms_t * F / tf * 1e-3), 1),
              "largest_relative_difference": float(((ours - ref_t).abs().max() / ref_t.abs().max()).item())})

out = {"tool": "tools/order_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "species": 2, "frames": F, "r_cut": args.rcut, "q_max": args.qmax, "bins": args.bins,
                    "q_bins": args.qbins, "cell_A": side * 2.65, "image_range": M}, "runs": lines}
for line in lines:
    print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
