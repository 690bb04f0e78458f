"""The interface task (alignn_amd.interface) timed.

1. The match launch alone: --pairs P random pairs of surface cells (lengths 2.5 - 4.5 A, angles 60 - 120 degrees) at the
   reference's defaults (max_area 500, ratio tolerance 1, ltol 0.05, atol 1 degree) through ``match_lattices``, the median of
   --runs timed calls after a warm-up, against the numpy restatement (tests/interface_ref.py) on the first --ref-pairs of them.
2. The batched call: B film / substrate pairs of crystals of --atoms atoms (synthetic.make_crystal), the tools/relax_time.py
   model, fmax = 0 so every structure takes exactly --steps steps, against one relax call per structure (the reference's shape:
   substrate, film, interface one after the other) on the structures the batched call built.
Prints one JSON line per measurement."""
import argparse, json, math, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, interface_energy, match_lattices, relax
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--ref-pairs", type=int, default=8)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--batches", default="1,8")
ap.add_argument("--atoms", type=int, default=4)
ap.add_argument("--thickness", type=float, default=4.0)
ap.add_argument("--max-area", type=float, default=150.0)
ap.add_argument("--tasks", default="match,energy")
args = ap.parse_args()
dev = "cuda"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_of(fn, runs):
    fn()  # warm-up
    return statistics.median(timed(fn)[0] for _ in range(max(3, runs)))


if "match" in args.tasks.split(","):
    from tests import interface_ref as ref

    rng = np.random.default_rng(7)

    def cell():
        a, b = rng.uniform(2.5, 4.5, 2)
        g, t = math.radians(rng.uniform(60.0, 120.0)), rng.uniform(0, 2 * math.pi)
        rot = np.array([[math.cos(t), math.sin(t)], [-math.sin(t), math.cos(t)]])
        return np.array([[a, 0.0], [b * math.cos(g), b * math.sin(g)]]) @ rot

    films, subs = np.stack([cell() for _ in range(args.pairs)]), np.stack([cell() for _ in range(args.pairs)])
    t_dev = median_of(lambda: match_lattices(films, subs, device=dev), args.runs)
    res = match_lattices(films, subs, device=dev)
    n_ref = min(args.ref_pairs, args.pairs)
    t0 = time.perf_counter()
    wants = [ref.match(films[p], subs[p]) for p in range(n_ref)]
    t_ref = (time.perf_counter() - t0) / n_ref
    same = all(w["status"] == res.status[p] and (w["status"] != 0 or (w["i"], w["j"], w["score"]) ==
                                                 (res.film_multiple[p], res.subs_multiple[p], res.score[p])) for p, w in enumerate(wants))
    print(json.dumps({"task": "match", "pairs": args.pairs, "matched": int((res.status == 0).sum()),
                      "device_call_s": round(t_dev, 5), "device_per_pair_s": round(t_dev / args.pairs, 7),
                      "numpy_restatement_per_pair_s": round(t_ref, 4), "restated_pairs": n_ref, "same_results": bool(same),
                      "speedup_per_pair": round(t_ref / (t_dev / args.pairs), 1)}), flush=True)

if "energy" in args.tasks.split(","):
    torch.manual_seed(0)
    model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                                 atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
    batches = [int(b) for b in args.batches.split(",")]

    def crystals(seed0):
        lats, pos, feats = [], [], []
        for i in range(max(batches)):
            lat, frac, _ = make_crystal(args.atoms, seed0 + i)
            lats.append(lat)
            pos.append(frac @ lat)
            feats.append(torch.randn(args.atoms, 92, device=dev))
        return lats, pos, feats

    film, subs = crystals(4321), crystals(8765)
    kw = dict(steps=args.steps, fmax=0.0, optimize_lattice=True)
    geo = dict(film_thickness=args.thickness, subs_thickness=args.thickness, max_area=args.max_area)
    masks = ([0] * 6, [0] * 6, [1, 1, 0, 0, 0, 1])
    for B in batches:
        pairs = [(b, (1, 0, 0), b, (1, 0, 0)) for b in range(B)]
        call = lambda **k: interface_energy(model, tuple(x[:B] for x in film), tuple(x[:B] for x in subs), pairs, **geo, **{**kw, **k})  # noqa: E731
        start = call(relax_structures=False)  # the structures as built
        feats_b = torch.cat(film[2][:B] + subs[2][:B])
        matched = [p for p in range(B) if start.status[p] == 0]

        def one_by_one(which):
            calls = 0
            for p in which:
                for q in range(3):
                    relax(model, [start.lattices[p][q]], [start.positions[p][q]], [feats_b[start.src[p][q].long()]],
                          cell_mask=masks[q], **kw)
                    calls += 1
            return calls

        t_b = median_of(call, args.runs)
        res = call()
        t_1 = median_of(lambda: one_by_one(matched), args.runs) if matched else float("nan")
        print(json.dumps({"task": "energy", "B": B, "atoms": args.atoms, "steps": args.steps, "matched_pairs": len(matched),
                          "structures": 3 * len(matched), "atoms_relaxed": int(sum(len(x) for p in matched for x in res.positions[p])),
                          "relax_calls": res.n_relax_calls, "batched_s": round(t_b, 4), "reference_shape_relax_calls": 3 * len(matched),
                          "reference_shape_s": round(t_1, 4), "speedup": round(t_1 / t_b, 2) if matched else None}), flush=True)
