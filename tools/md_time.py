"""Batched MD (alignn_amd.run_md) timed per step: B in {1, 16, 64} crystals of 60 atoms (synthetic.make_crystal), the
tools/md_step.py model, at 300 K from a Maxwell-Boltzmann start (--ensemble: any of run_md's; npt_berendsen at 1 bar with a
compressibility of 1e-6 / bar; nvt_nose_hoover with ttime 25 fs, npt_nose_hoover with that, ptime 250 fs and 1 bar).  Beside each batch, the same structures run one at a
time through the same function - what the reference's per-structure ForceField MD amounts to - and both with and without
replay (md.GraphedForceField).  Prints one JSON line per B."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, run_md
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batches", default="1,16,64")
ap.add_argument("--atoms", type=int, default=60)
ap.add_argument("--ensemble", default="nvt_langevin")
ap.add_argument("--modes", default="eager,replay")
ap.add_argument("--repeats", type=int, default=1)  # timed runs per figure after the warm-up; the median is reported
args = ap.parse_args()
dev = "cuda"
torch.manual_seed(0)
model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                             atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
Bmax = max(int(b) for b in args.batches.split(","))
lats, pos, feats, masses = [], [], [], []
for i in range(Bmax):
    lat, frac, _ = make_crystal(args.atoms, 4321 + i)
    lats.append(lat)
    pos.append(frac @ lat)
    feats.append(torch.randn(args.atoms, 92, device=dev))
    masses.append(np.random.default_rng(i).uniform(10.0, 100.0, args.atoms))
kw = dict(ensemble=args.ensemble, timestep=1.0, steps=args.steps, temperature_K=300.0, friction=0.01,
          initial_temperature_K=300.0, trajectory=False)
if args.ensemble == "npt_berendsen":
    kw.update(pressure=1.0, compressibility=1e-6)
if args.ensemble == "nvt_nose_hoover":
    kw.update(ttime=25.0)
if args.ensemble == "npt_nose_hoover":
    kw.update(ttime=25.0, ptime=250.0, pressure=1.0)


def timed(B, one_at_a_time, replay):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if one_at_a_time:
        evals = sum(run_md(model, lats[i:i + 1], pos[i:i + 1], feats[i:i + 1], masses[i:i + 1], seed=i, replay=replay,
                           **kw).n_evals for i in range(B))
    else:
        evals = run_md(model, lats[:B], pos[:B], feats[:B], masses[:B], seed=list(range(B)), replay=replay, **kw).n_evals
    torch.cuda.synchronize()
    return time.perf_counter() - t0, evals


run_md(model, lats[:2], pos[:2], feats[:2], masses[:2], **{**kw, "steps": 3})  # warm-up: code objects, allocator, lattice tables
for B in [int(b) for b in args.batches.split(",")]:
    line = {"B": B, "atoms": args.atoms, "steps": args.steps, "ensemble": args.ensemble}
    line["repeats"] = args.repeats
    for tag in args.modes.split(","):
        replay = tag == "replay"
        timed(B, False, replay)  # warm-up of this batch's shapes
        runs_b = [timed(B, False, replay) for _ in range(args.repeats)]
        runs_1 = [timed(B, True, replay) for _ in range(args.repeats)]
        (t_b, ev_b), (t_1, ev_1) = sorted(runs_b)[len(runs_b) // 2], sorted(runs_1)[len(runs_1) // 2]
        line.update({f"{tag}_batched_ms_per_step": round(1e3 * t_b / ev_b, 3),
                     f"{tag}_batched_structure_steps_per_s": round(B * args.steps / t_b, 1),
                     f"{tag}_one_at_a_time_structure_steps_per_s": round(B * args.steps / t_1, 1),
                     f"{tag}_speedup": round(t_1 / t_b, 2)})
    print(json.dumps(line), flush=True)
