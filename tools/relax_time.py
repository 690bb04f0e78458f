"""Batched FIRE relaxation (alignn_amd.relax) timed per step: B in {1, 16, 64} crystals of 60 atoms (synthetic.make_crystal),
the tools/md_step.py model, fmax = 0 so every structure takes exactly --steps steps.  Beside each batch, the same structures
relaxed one at a time through the same function - what the reference's per-structure optimize_atoms loop amounts to.
--cell relaxes the cells too (optimize_lattice=True: ExpCellFilter, alignn_fire_step with the filter's state).  --fixed,
--slab-mask, --pressure, --hydrostatic and --constant-volume switch the constraints on (--constraints: all of them; they
imply --cell except --fixed).  --repeats R: the batched time is the median of R runs, their spread is printed too.
--skip-serial leaves the one-at-a-time loop out.  Prints one JSON line per B."""
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, relax
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batches", default="1,16,64")
ap.add_argument("--atoms", type=int, default=60)
ap.add_argument("--cell", action="store_true", help="optimize_lattice=True")
ap.add_argument("--fixed", action="store_true", help="hold the first quarter of every structure's atoms (FixAtoms)")
ap.add_argument("--slab-mask", action="store_true", help="cell_mask=[1, 1, 0, 0, 0, 1]")
ap.add_argument("--pressure", type=float, default=0.0, help="scalar_pressure, eV/A^3")
ap.add_argument("--hydrostatic", action="store_true", help="hydrostatic_strain=True")
ap.add_argument("--constant-volume", action="store_true", help="constant_volume=True")
ap.add_argument("--constraints", action="store_true", help="all of the above, with --pressure 0.01 unless given")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--skip-serial", action="store_true")
args = ap.parse_args()
if args.constraints:
    args.fixed = args.slab_mask = args.hydrostatic = args.constant_volume = True
    args.pressure = args.pressure or 0.01
args.cell = args.cell or args.slab_mask or args.hydrostatic or args.constant_volume or args.pressure != 0.0
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


def options(lo, hi):
    """The keyword arguments of relax for structures lo .. hi: only what the flags switch on (none: the call as it always was)."""
    kw = dict(optimize_lattice=args.cell)
    if args.fixed:
        kw["fixed"] = [torch.arange(args.atoms) < args.atoms // 4 for _ in range(lo, hi)]
    if args.slab_mask:
        kw["cell_mask"] = [1, 1, 0, 0, 0, 1]
    if args.pressure != 0.0:
        kw["scalar_pressure"] = args.pressure
    if args.hydrostatic:
        kw["hydrostatic_strain"] = True
    if args.constant_volume:
        kw["constant_volume"] = True
    return kw


def timed(B, one_at_a_time):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if one_at_a_time:
        evals = sum(relax(model, lats[i:i + 1], pos[i:i + 1], feats[i:i + 1], fmax=0.0, steps=args.steps,
                          **options(i, i + 1)).n_evals for i in range(B))
    else:
        evals = relax(model, lats[:B], pos[:B], feats[:B], fmax=0.0, steps=args.steps, **options(0, B)).n_evals
    torch.cuda.synchronize()
    return time.perf_counter() - t0, evals


relax(model, lats[:2], pos[:2], feats[:2], fmax=0.0, steps=3, **options(0, 2))  # warm-up: code objects, allocator, lattice tables
for B in [int(b) for b in args.batches.split(",")]:
    timed(B, False)  # warm-up of this batch's shapes
    runs = [timed(B, False) for _ in range(args.repeats)]
    t_b, ev_b = statistics.median(r[0] for r in runs), runs[0][1]
    line = {"B": B, "atoms": args.atoms, "steps": args.steps, "cell": args.cell,
            "constraints": sorted(k for k in options(0, 1) if k != "optimize_lattice"),
            "batched_ms_per_step": round(1e3 * t_b / ev_b, 3),
            "batched_ms_per_step_runs": [round(1e3 * r[0] / r[1], 3) for r in runs],
            "batched_structure_steps_per_s": round(B * args.steps / t_b, 1)}
    if not args.skip_serial:
        t_1, ev_1 = timed(B, True)
        line.update({"one_at_a_time_ms_per_structure_step": round(1e3 * t_1 / ev_1, 3),
                     "one_at_a_time_structure_steps_per_s": round(B * args.steps / t_1, 1),
                     "speedup": round(t_1 / t_b, 2)})
    print(json.dumps(line), flush=True)
