"""Batched FIRE relaxation (alignn_amd.relax) timed per step: B in {1, 16, 64} crystals of 60 atoms (synthetic.make_crystal),
the tools/md_step.py model, fmax = 0 so every structure takes exactly --steps steps.  Beside each batch, the same structures
relaxed one at a time through the same function - what the reference's per-structure optimize_atoms loop amounts to.
--cell relaxes the cells too (optimize_lattice=True: ExpCellFilter, alignn_fire_step with the filter's state).  Prints one JSON
line per B."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, relax
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batches", default="1,16,64")
ap.add_argument("--atoms", type=int, default=60)
ap.add_argument("--cell", action="store_true", help="optimize_lattice=True")
args = ap.parse_args()
dev = "cuda"
torch.manual_seed(0)
model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                             atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
Bmax = max(int(b) for b in args.batches.split(","))
lats, pos, feats = [], [], []
for i in range(Bmax):
    lat, frac, _ = make_crystal(args.atoms, 4321 + i)
    lats.append(lat)
    pos.append(frac @ lat)
    feats.append(torch.randn(args.atoms, 92, device=dev))


def timed(B, one_at_a_time):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if one_at_a_time:
        evals = sum(relax(model, lats[i:i + 1], pos[i:i + 1], feats[i:i + 1], fmax=0.0, steps=args.steps,
                          optimize_lattice=args.cell).n_evals for i in range(B))
    else:
        evals = relax(model, lats[:B], pos[:B], feats[:B], fmax=0.0, steps=args.steps, optimize_lattice=args.cell).n_evals
    torch.cuda.synchronize()
    return time.perf_counter() - t0, evals


relax(model, lats[:2], pos[:2], feats[:2], fmax=0.0, steps=3, optimize_lattice=args.cell)  # warm-up: code objects, allocator, lattice tables
for B in [int(b) for b in args.batches.split(",")]:
    timed(B, False)  # warm-up of this batch's shapes
    t_b, ev_b = timed(B, False)
    t_1, ev_1 = timed(B, True)
    print(json.dumps({"B": B, "atoms": args.atoms, "steps": args.steps, "cell": args.cell,
                      "batched_ms_per_step": round(1e3 * t_b / ev_b, 3),
                      "batched_structure_steps_per_s": round(B * args.steps / t_b, 1),
                      "one_at_a_time_ms_per_structure_step": round(1e3 * t_1 / ev_1, 3),
                      "one_at_a_time_structure_steps_per_s": round(B * args.steps / t_1, 1),
                      "speedup": round(t_1 / t_b, 2)}), flush=True)
