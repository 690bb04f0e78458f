"""The van Hove analysis (alignn_amd.vanhove) timed per function on a synthetic trajectory, so no model is needed: --structs B
structures of --atoms atoms with two species, --frames frames of a random walk about a simple-cubic-like lattice (spacing 2.5 A);
``van_hove_self`` with the lags 0 .. --lag, three |q| and origin stride 1; ``van_hove_distinct`` with --distinct-lags log-spaced
lags and origin stride --distinct-stride; ``intermediate_scattering`` with the lags 0 .. --lag inside --qmax and origin stride 1.

Per function: the median of --repeats calls timed with device events after a warm-up, and the terms (origin x atom), pair images
(ordered origin, i, j, image examined) or products (origin x vector x lag) per second.  Beside each, the same quantity as plain
torch expressions on the same device: a loop over the lags with ``histc`` for the self part; per origin the dense distances of all
structures to every image and ``histc`` for the distinct part (every pair, no species rows; timed on --torch-origins origins of
one lag and scaled to all); ``exp(i q . r)`` by a matrix product and a loop over the lags for F(q, t) (the total only; timed on one
structure and scaled to all).  Writes one JSON file (default profiles/vanhove_time.json) and prints it.  All in one process."""
import argparse, itertools, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import intermediate_scattering, van_hove_distinct, van_hove_self
from tests import traj_ref

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=16)
ap.add_argument("--atoms", type=int, default=200)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--rmax", type=float, default=8.0)
ap.add_argument("--self-rmax", type=float, default=2.0)
ap.add_argument("--bins", type=int, default=200)
ap.add_argument("--lag", type=int, default=500)
ap.add_argument("--distinct-lags", type=int, default=16)
ap.add_argument("--distinct-stride", type=int, default=10)
ap.add_argument("--qmax", type=float, default=3.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--torch-origins", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vanhove_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("vanhove_time: no GPU; nothing is measured without one")
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
pos = torch.tensor(pos_h, device=dev)
cells = torch.tensor(np.tile(cell[None], (B, 1, 1)), device=dev)
ns = [n] * B
M = traj_ref.image_range(cell, args.rmax)
images = int(np.prod([2 * m + 1 for m in M]))
QS = (0.8, 1.6, 2.5)
d_lags = []
for v in np.logspace(0.0, np.log10(K), args.distinct_lags):  # log-spaced, and distinct where two round to the same frame
    d_lags.append(max(int(round(v)), d_lags[-1] + 1 if d_lags else 1))
n_or = lambda k, stride: (F - 1 - k) // stride + 1


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
mass_t = torch.tensor(np.concatenate(masses_h), device=dev)
# --- the self part ---------------------------------------------------------------------------------------------------------------------
terms = B * n * sum(n_or(k, 1) for k in range(K + 1))
ours_self = lambda: van_hove_self(pos, ns, species_h, masses_h, r_max=args.self_rmax, n_bins=args.bins, max_lag=K, q=QS)
ms, runs = timed(ours_self)
lines.append({"what": f"van_hove_self (centre of mass + histograms, moments and fs at {len(QS)} q + finish), lags 0 .. {K}", "ms": round(ms, 3),
              "ms_runs": runs, "terms": terms, "terms_per_s": round(terms / (ms * 1e-3), 1)})


def torch_self():
    x = pos.view(F, B, n, 3)
    c = (x * mass_t.view(1, B, n, 1)).sum(2) / mass_t.view(B, n).sum(1)[None, :, None]
    q = torch.tensor(QS, device=dev, dtype=torch.float64)
    hist = torch.zeros(K + 1, args.bins, dtype=torch.float64, device=dev)
    m2, fs = torch.zeros(K + 1, B, dtype=torch.float64, device=dev), torch.zeros(K + 1, B, len(QS), dtype=torch.float64, device=dev)
    for k in range(K + 1):
        d = (x[k:] - x[:F - k]) - (c[k:] - c[:F - k])[:, :, None, :]
        r2 = (d * d).sum(-1)
        r = torch.sqrt(r2)
        hist[k] = torch.histc(r[r < args.self_rmax], bins=args.bins, min=0.0, max=args.self_rmax)
        m2[k] = r2.mean((0, 2))
        fs[k] = torch.special.sinc(r[..., None] * (q / np.pi)).mean((0, 2))
    return hist, m2, fs


ms, runs = timed(torch_self, repeats=3)
res, (hist, m2, fs) = ours_self(), torch_self()
lines.append({"what": "the same as torch expressions (a loop over the lags; every atom only)", "ms": round(ms, 3), "ms_runs": runs,
              "terms_per_s": round(terms / (ms * 1e-3), 1),
              "histograms_differ_in": int((res.counts[:, 0].sum(0).double() - hist).abs().sum().item()),
              "largest_difference_of_fs": float((res.fs[:, 0].permute(1, 0, 2) - fs).abs().max().item())})

# --- the distinct part -----------------------------------------------------------------------------------------------------------------
origins = sum(n_or(k, args.distinct_stride) for k in d_lags)
pairs = origins * B * n * n * images
ours_distinct = lambda: van_hove_distinct(pos, cells, ns, species_h, r_max=args.rmax, n_bins=args.bins, lags=d_lags,
                                          origin_stride=args.distinct_stride)
ms, runs = timed(ours_distinct)
lines.append({"what": f"van_hove_distinct (counts + finish + the status word's read-back), {len(d_lags)} lags {d_lags}, origin stride "
                      f"{args.distinct_stride}", "ms": round(ms, 3), "ms_runs": runs, "origins": origins, "pair_images": pairs,
              "pair_images_per_s": round(pairs / (ms * 1e-3), 1), "images_per_pair": images})
shifts = torch.tensor(np.array(list(itertools.product(*[range(-m, m + 1) for m in M])), dtype=np.float64) @ cell, device=dev)
inv = torch.linalg.inv(cells)
k_t = d_lags[len(d_lags) // 2]
n_t = min(args.torch_origins, n_or(k_t, args.distinct_stride))


def torch_distinct():
    hist = torch.zeros(args.bins, dtype=torch.float64, device=dev)
    eye = torch.eye(n, device=dev)[None, :, :, None] > 0
    for o in range(n_t):
        t = o * args.distinct_stride
        xa, xb = pos[t].view(B, n, 3), pos[t + k_t].view(B, n, 3)
        dp = xb[:, None, :, :] - xa[:, :, None, :]
        df = dp @ inv[:, None]
        shift = torch.round(df)
        d0 = (df - shift) @ cells[:, None]
        d = d0[:, :, :, None, :] + shifts[None, None, None]
        r = torch.sqrt((d * d).sum(-1))
        own = eye & ((shift @ cells[:, None])[:, :, :, None, :] - shifts[None, None, None]).abs().sum(-1).lt(1e-9)
        r = torch.where(own, torch.full_like(r, 2.0 * args.rmax), r)
        hist += torch.histc(r[r < args.rmax], bins=args.bins, min=0.0, max=args.rmax)
    return hist


ms_t, runs_t = timed(torch_distinct, repeats=3)
lines.append({"what": f"the same as torch expressions (every pair only; {n_t} origins of lag {k_t} timed, scaled to {origins})",
              "ms": round(ms_t * origins / n_t, 3), "ms_runs_of_the_timed_origins": runs_t,
              "pair_images_per_s": round(pairs / (ms_t * origins / n_t * 1e-3), 1)})
sub = pos[:k_t + (n_t - 1) * args.distinct_stride + 1].contiguous()
got = van_hove_distinct(sub, cells, ns, None, r_max=args.rmax, n_bins=args.bins, lags=[k_t], origin_stride=args.distinct_stride)
lines[-1]["histograms_differ_in"] = int((got.counts[:, 0, 0].sum(0).double() - torch_distinct()).abs().sum().item())  # (a pair at a bin edge may move)

# --- the intermediate scattering function -------------------------------------------------------------------------------------------------
ours_fqt = lambda: intermediate_scattering(pos, cells, ns, species_h, q_max=args.qmax, n_bins=args.bins, max_lag=K)
res = ours_fqt()
V = int(res.hkl[0].shape[0])
products = B * V * sum(n_or(k, 1) for k in range(K + 1))
ms, runs = timed(ours_fqt)
lines.append({"what": f"intermediate_scattering (vectors + modes + correlate + bin), lags 0 .. {K}, {V} vectors per structure",
              "ms": round(ms, 3), "ms_runs": runs, "products": products, "products_per_s": round(products / (ms * 1e-3), 1),
              "workspace_bytes": 16 * F * 2 * B * V})
qv = (2.0 * np.pi) * (res.hkl[0].double() @ torch.linalg.inv(cells[0]).T)  # [V, 3]


def torch_fqt():
    rho = torch.exp(1j * (pos[:, :n] @ qv.T)).sum(1)  # [F, V], one structure
    out = torch.empty(K + 1, V, dtype=torch.float64, device=dev)
    for k in range(K + 1):
        out[k] = (rho[k:] * rho[:F - k].conj()).real.mean(0) / n
    return out


ms_t, runs_t = timed(torch_fqt, repeats=3)
lines.append({"what": f"the same as torch expressions (the total only; one structure timed, scaled to {B})", "ms": round(ms_t * B, 3),
              "ms_runs_of_one_structure": runs_t, "products_per_s": round(products / (ms_t * B * 1e-3), 1),
              "largest_difference": float((res.f_vectors[0][0] - torch_fqt()).abs().max().item())})

out = {"tool": "tools/vanhove_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "species": 2, "frames": F, "r_max": args.rmax, "self_r_max": args.self_rmax, "bins": args.bins,
                    "max_lag": K, "distinct_lags": d_lags, "distinct_stride": args.distinct_stride, "q_max": args.qmax, "q": QS,
                    "cell_A": side * 2.5, "image_range": M}, "runs": lines}
for line in lines:
    print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
