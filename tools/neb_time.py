"""Batched nudged elastic band (alignn_amd.neb) timed per FIRE step: B bands of --images interior images of --atoms atoms
(synthetic.make_crystal, the final image the initial one with one atom displaced by 0.4 A), the tools/relax_time.py model,
fmax = 0 so every band takes exactly --steps steps.  Beside each batch, the same number of image evaluations made one image per
model call through ``relax(..., steps=0)`` - what ASE's NEB around a calculator amounts to in model calls (its optimiser and
projection, which cost next to nothing, are left out, so the loop is a lower bound of that run).  --repeats R: the batched time is
the median of R runs, their spread is written too.  Writes one JSON file (default profiles/neb_time.json) and prints it."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, neb, relax
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batches", default="1,8")
ap.add_argument("--atoms", type=int, default=60)
ap.add_argument("--images", type=int, default=5, help="interior images per band")
ap.add_argument("--method", default="aseneb")
ap.add_argument("--climb", action="store_true")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "neb_time.json"))
args = ap.parse_args()
dev = "cuda"
torch.manual_seed(0)
model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                             atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
batches = [int(b) for b in args.batches.split(",")]
lats, first, last, feats = [], [], [], []
for i in range(max(batches)):
    lat, frac, _ = make_crystal(args.atoms, 4321 + i)
    p = np.asarray(frac @ lat, dtype=np.float64)
    q = p.copy()
    q[0] += np.array([0.4, 0.0, 0.0])
    lats.append(lat)
    first.append(p)
    last.append(q)
    feats.append(torch.randn(args.atoms, 92, device=dev))
kw = dict(n_images=args.images, method=args.method, climb=args.climb, fmax=0.0, steps=args.steps)


def batched(B):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = neb(model, lats[:B], first[:B], last[:B], feats[:B], **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def one_image_per_call(B, res):
    """The image evaluations of the batched run (the endpoints once, every interior image at every evaluation), one per model
    call, on the final images."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    calls = 0
    for b in range(B):
        for j in (0, args.images + 1):
            relax(model, lats[b:b + 1], [res.positions[b][j]], feats[b:b + 1], steps=0)
            calls += 1
        for _ in range(res.n_evals):
            for j in range(1, args.images + 1):
                relax(model, lats[b:b + 1], [res.positions[b][j]], feats[b:b + 1], steps=0)
                calls += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, calls


neb(model, lats[:1], first[:1], last[:1], feats[:1], **dict(kw, steps=2))  # warm-up: code objects, allocator, lattice tables
lines = []
for B in batches:
    batched(B)  # warm-up of this batch's shapes
    runs = [batched(B) for _ in range(args.repeats)]
    t_b, res = statistics.median(r[0] for r in runs), runs[0][1]
    t_1, calls = one_image_per_call(B, res)
    lines.append({"B": B, "atoms": args.atoms, "interior_images": args.images, "steps": args.steps, "method": args.method,
                  "climb": args.climb, "band_evaluations": res.n_evals, "batched_s": round(t_b, 4),
                  "batched_s_runs": [round(r[0], 4) for r in runs], "batched_ms_per_step": round(1e3 * t_b / res.n_evals, 3),
                  "one_image_per_call_s": round(t_1, 4), "one_image_per_call_model_calls": calls,
                  "one_image_per_call_ms_per_call": round(1e3 * t_1 / calls, 3), "ratio": round(t_1 / t_b, 2)})
    print(json.dumps(lines[-1]), flush=True)
out = {"tool": "tools/neb_time.py", "device": torch.cuda.get_device_name(0), "runs": lines}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
