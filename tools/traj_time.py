"""Trajectory analysis (alignn_amd.trajectory) timed per kernel on a synthetic trajectory, so no model is needed: --structs B
structures of --atoms atoms with two species, --frames frames of a random walk about a simple-cubic-like lattice (spacing 2.5 A);
g(r) with --rmax and --bins, MSD and VACF with --lag lags and origin stride 1.

Per function: the median of --repeats launches timed with device events after a warm-up, the pairs (ordered i, j, image triples
examined) or terms (origin x atom) per second, the bytes the algorithm must read (the frames once) and the bytes the kernel asks
the memory system for.  Beside each, the same quantity as plain torch expressions on the same device: per frame the dense
distances of all structures to every image and ``histc`` (every pair, no species rows; timed on --torch-frames frames and scaled
to all), and a loop over the lags for MSD and VACF.  Last, the numpy restatement (tests/traj_ref.py) on the host for one
structure, on --host-frames frames and --host-lags lags, as rates.  Writes one JSON file (default profiles/traj_time.json) and
prints it.  All in one process."""
import argparse, itertools, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import msd, rdf, vacf
from tests import traj_ref

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=16)
ap.add_argument("--atoms", type=int, default=200)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--rmax", type=float, default=8.0)
ap.add_argument("--bins", type=int, default=400)
ap.add_argument("--lag", type=int, default=500)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--torch-frames", type=int, default=50)
ap.add_argument("--host-frames", type=int, default=3)
ap.add_argument("--host-lags", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("traj_time: no GPU; nothing is measured without one")
dev = "cuda"
B, n, F, K = args.structs, args.atoms, args.frames, args.lag
rng = np.random.default_rng(7)
side = int(np.ceil(n ** (1 / 3)))
grid = np.array(list(itertools.product(range(side), repeat=3)), dtype=np.float64)[:n] * 2.5
cell = np.eye(3) * side * 2.5
walk = np.cumsum(rng.normal(0.0, 0.02, (F, B * n, 3)), axis=0)
pos_h = np.tile(grid, (B, 1))[None] + walk
masses_h = [np.where(np.arange(n) % 2 == 0, 6.94, 16.0) for _ in range(B)]
species_h = [np.where(np.arange(n) % 2 == 0, 3, 8) for _ in range(B)]
mom_h = rng.normal(0.0, 1.0, (F, B * n, 3)) * np.sqrt(np.concatenate(masses_h))[None, :, None]
pos, mom = torch.tensor(pos_h, device=dev), torch.tensor(mom_h, device=dev)
cells = torch.tensor(np.tile(cell[None], (B, 1, 1)), device=dev)
ns = [n] * B
M = traj_ref.image_range(cell, args.rmax)
images = int(np.prod([2 * m + 1 for m in M]))


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
# --- g(r) ----------------------------------------------------------------------------------------------------------------------------
pairs = F * B * (n * n * images - n)
tiles = -(-n // 64)
ms, runs = timed(lambda: rdf(pos, cells, ns, species_h, r_max=args.rmax, n_bins=args.bins))
lines.append({"what": "rdf (counts + normalise + the status word's read-back)", "ms": round(ms, 3), "ms_runs": runs,
              "pair_images": pairs, "pair_images_per_s": round(pairs / (ms * 1e-3), 1), "images_per_pair": images,
              "compulsory_bytes": F * B * n * 24, "requested_bytes": F * B * tiles * (64 + n) * 28})

shifts = torch.tensor(np.array(list(itertools.product(*[range(-m, m + 1) for m in M])), dtype=np.float64) @ cell, device=dev)
inv = torch.linalg.inv(cells)


def torch_rdf(frames):
    hist = torch.zeros(args.bins, dtype=torch.float64, device=dev)
    own = (torch.eye(n, device=dev)[None, :, :, None] > 0) & (shifts.abs().sum(1) == 0)[None, None, None, :]
    for f in range(frames):
        x = pos[f].view(B, n, 3)
        dp = x[:, None, :, :] - x[:, :, None, :]
        df = dp @ inv[:, None]
        d0 = (df - torch.round(df)) @ cells[:, None]
        d = d0[:, :, :, None, :] + shifts[None, None, None]
        r = torch.sqrt((d * d).sum(-1))
        r = torch.where(own, torch.full_like(r, 2.0 * args.rmax), r)
        hist += torch.histc(r[r < args.rmax], bins=args.bins, min=0.0, max=args.rmax)
    return hist


tf = min(args.torch_frames, F)
ms_t, runs_t = timed(lambda: torch_rdf(tf), repeats=3)
lines.append({"what": f"rdf as torch expressions (every pair only, {tf} frames timed, scaled to {F})", "ms": round(ms_t * F / tf, 3),
              "ms_runs_of_the_timed_frames": runs_t, "pair_images_per_s": round(pairs / (ms_t * F / tf * 1e-3), 1)})
got = rdf(pos[:tf].contiguous(), cells, ns, None, r_max=args.rmax, n_bins=args.bins).counts[:, 0].sum(0)
lines[-1]["histograms_differ_in"] = int((got.double() - torch_rdf(tf)).abs().sum().item())  # (pairs at a bin edge may move)

# --- MSD and VACF ----------------------------------------------------------------------------------------------------------------------
terms = B * n * sum(F - k for k in range(K + 1))
for name, fn in (("msd", lambda: msd(pos, ns, species_h, masses_h, max_lag=K)), ("vacf", lambda: vacf(mom, ns, species_h, masses_h, max_lag=K))):
    ms, runs = timed(fn)
    lines.append({"what": name + (" (centre of mass + correlation)" if name == "msd" else ""), "ms": round(ms, 3), "ms_runs": runs,
                  "terms": terms, "terms_per_s": round(terms / (ms * 1e-3), 1), "compulsory_bytes": F * B * n * 24,
                  "requested_bytes": terms * 48})

mass_t = torch.tensor(np.concatenate(masses_h), device=dev)
member = torch.stack([torch.ones(n, device=dev, dtype=torch.float64)] + [torch.tensor((species_h[0] == z).astype(np.float64), device=dev) for z in (3, 8)])


def torch_msd():
    x = pos.view(F, B, n, 3)
    c = (x * mass_t.view(1, B, n, 1)).sum(2) / mass_t.view(B, n).sum(1)[None, :, None]
    out = torch.empty(B, 3, K + 1, 3, dtype=torch.float64, device=dev)
    for k in range(K + 1):
        d = (x[k:] - x[:F - k]) - (c[k:] - c[:F - k])[:, :, None, :]
        per_atom = (d * d).sum(0)  # [B, n, 3]
        out[:, :, k] = torch.einsum("gn,bnc->bgc", member, per_atom) / ((F - k) * member.sum(1))[None, :, None]
    return out


def torch_vacf():
    v = (mom / mass_t[None, :, None]).view(F, B, n, 3)
    out = torch.empty(B, 3, K + 1, dtype=torch.float64, device=dev)
    for k in range(K + 1):
        per_atom = (v[k:] * v[:F - k]).sum(-1).sum(0)  # [B, n]
        out[:, :, k] = torch.einsum("gn,bn->bg", member, per_atom) / ((F - k) * member.sum(1))[None, :]
    return out


for name, fn, ours in (("msd", torch_msd, lambda: msd(pos, ns, species_h, masses_h, max_lag=K).msd),
                       ("vacf", torch_vacf, lambda: vacf(mom, ns, species_h, masses_h, max_lag=K).vacf)):
    ms, runs = timed(fn, repeats=3)
    a, b = ours(), fn()
    lines.append({"what": f"{name} as torch expressions (a loop over the lags)", "ms": round(ms, 3), "ms_runs": runs,
                  "terms_per_s": round(terms / (ms * 1e-3), 1),
                  "largest_relative_difference": float(((a - b).abs().max() / b.abs().max()).item())})

# --- the restatement on the host, one structure ------------------------------------------------------------------------------------------
rank, _ = traj_ref.groups(species_h[0], n)
hf, hk = min(args.host_frames, F), min(args.host_lags, F - 1)
t0 = time.perf_counter()
traj_ref.rdf_counts(pos_h[:hf, :n], cell, rank, 2, args.rmax, args.bins)
t_r = time.perf_counter() - t0
t0 = time.perf_counter()
traj_ref.msd(pos_h[:, :n], rank, 2, masses_h[0], hk)
t_m = time.perf_counter() - t0
lines.append({"what": f"numpy restatement on the host, one structure ({hf} frames of g(r), {hk + 1} lags of MSD)",
              "rdf_s": round(t_r, 3), "pair_images_per_s": round(hf * (n * n * images - n) / t_r, 1), "msd_s": round(t_m, 3),
              "terms_per_s": round(n * sum(F - k for k in range(hk + 1)) / t_m, 1)})

out = {"tool": "tools/traj_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "species": 2, "frames": F, "r_max": args.rmax, "bins": args.bins, "max_lag": K,
                    "origin_stride": 1, "cell_A": side * 2.5, "image_range": M}, "runs": lines}
for line in lines:
    print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
