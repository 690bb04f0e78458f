"""The defect tasks (alignn_amd.defects) timed: B crystals of --atoms atoms (synthetic.make_crystal), the tools/relax_time.py
model, fmax = 0 so every structure takes exactly --steps steps.  Batched: one vacancy_formation / surface_energy call.  Reference
shape: one relax call per structure, as the reference's loops run (alignn/ff/ff.py:808-981) - for vacancies the pristine
supercell relaxed once per defect, for surfaces the parent and then slab after slab - on the structures the batched call built.
--classes C: site labels arange(n) % C (C defects per parent).  --hkl: the Miller indices of every parent.  Prints one JSON line
per task and B."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, relax, surface_energy, vacancy_formation
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batches", default="1,8")
ap.add_argument("--atoms", type=int, default=8)
ap.add_argument("--classes", type=int, default=4)
ap.add_argument("--supercell", default="2,2,2")
ap.add_argument("--hkl", default="100,110,111,211")
ap.add_argument("--thickness", type=float, default=12.0)
ap.add_argument("--vacuum", type=float, default=12.0)
ap.add_argument("--tasks", default="vacancy,surface")
args = ap.parse_args()
dev = "cuda"
torch.manual_seed(0)
model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                             atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
batches = [int(b) for b in args.batches.split(",")]
sc = tuple(int(v) for v in args.supercell.split(","))
hkls = [tuple(int(c) for c in h) for h in args.hkl.split(",")]  # (single digits, none negative)
lats, pos, feats = [], [], []
for i in range(max(batches)):
    lat, frac, _ = make_crystal(args.atoms, 4321 + i)
    lats.append(lat)
    pos.append(frac @ lat)
    feats.append(torch.randn(args.atoms, 92, device=dev))
labels = [np.arange(args.atoms) % args.classes] * max(batches)
kw = dict(steps=args.steps, fmax=0.0, optimize_lattice=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_by_one(res, B, repeat_first):
    """One relax call per structure of the batched result ``res`` (the structures as built: its ``src`` gives the features; the
    start positions are rebuilt by a steps = 0 call).  ``repeat_first``: job 0 of a parent once per further job."""
    calls = 0
    for s in range(B):
        jobs = list(range(len(res.positions[s])))
        order = [j for k in jobs[1:] for j in (0, k)] if repeat_first else jobs
        for j in order:
            f = torch.cat(feats)[res.src[s][j].long()]
            relax(model, [start.lattices[s][j]], [start.positions[s][j]], [f], **kw, **extra)
            calls += 1
    return calls


for task in args.tasks.split(","):
    for B in batches:
        extra = {} if task == "vacancy" else dict(cell_mask=[1, 1, 0, 0, 0, 1])
        if task == "vacancy":
            call = lambda **k: vacancy_formation(model, lats[:B], pos[:B], feats[:B], site_labels=labels[:B], supercell=sc, **{**kw, **k})
        else:
            call = lambda **k: surface_energy(model, lats[:B], pos[:B], feats[:B], miller_indices=hkls, thickness=args.thickness,
                                              vacuum=args.vacuum, **{**kw, **extra, **k})
        start = call(relax_structures=False)  # the structures as built (and the warm-up of this batch's shapes)
        call()
        t_b, res = timed(call)
        one_by_one(res, 1, task == "vacancy")  # warm-up
        t_1, calls = timed(lambda: one_by_one(res, B, task == "vacancy"))
        n_jobs = sum(len(p) for p in res.positions)
        print(json.dumps({"task": task, "B": B, "atoms": args.atoms, "steps": args.steps, "structures": n_jobs,
                          "atoms_relaxed": int(sum(len(x) for p in res.positions for x in p)), "relax_calls": res.n_relax_calls,
                          "batched_s": round(t_b, 4), "reference_shape_relax_calls": calls, "reference_shape_s": round(t_1, 4),
                          "speedup": round(t_1 / t_b, 2)}), flush=True)
