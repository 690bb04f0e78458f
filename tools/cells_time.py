"""The conventional and primitive cells (alignn_amd.cells) timed at the shape of tools/sym_time.py: --structs structures of 200
atoms, no model needed.  One half has a single species - 5 x 5 x 4 supercells of hcp, 100 pure translations each, so the
conventional cell goes through the reduced primitive cell and a second, small symmetry search; the other half is the same 200
sites decorated at random with 4 species: primitive as given, triclinic.  The lattice constants differ from structure to
structure.

Per measurement the median of --repeats calls timed with device events after a warm-up call: ``conventional_cell`` and
``primitive_cell`` with the ``SymmetryResult`` passed in (the cells alone: the launches, the read-back in between and, for the
supercells, the second round with its own search), ``conventional_cell`` with the search included, and the same structures one
per call.  Writes one JSON file (default profiles/cells_time.json) and prints it.  All in one process."""
import argparse, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import conventional_cell, find_symmetry, primitive_cell
from tests import sym_ref

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--symprec", type=float, default=1e-3)
ap.add_argument("--skip-single", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("cells_time: no GPU; nothing is measured without one")
B = args.structs
rng = np.random.default_rng(7)
lats, poss, zs = [], [], []
for b in range(B):
    a = 3.2 * (1.0 + 0.002 * b)
    cell = sym_ref.hexagonal_cell(a, 1.633 * a)
    A, pos, z = sym_ref.supercell(cell, np.array([[1 / 3, 2 / 3, 0.25], [2 / 3, 1 / 3, 0.75]]) @ cell, np.array([12, 12]), (5, 5, 4))
    lats.append(A)
    poss.append(pos)
    zs.append(z if b < B // 2 else rng.integers(0, 4, len(pos)) + 20)
n = len(poss[0])


def timed(fn, repeats=args.repeats):
    """Median (and all) of ``repeats`` calls in ms by device events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), [round(m, 3) for m in ms]


lines = []
sym = find_symmetry(lats, poss, zs, symprec=args.symprec)
res = conventional_cell(lats, poss, zs, symprec=args.symprec, sym=sym)
what = {"atoms_out": [res.ns[0], res.ns[-1]], "centring": [res.centring[0], res.centring[-1]],
        "crystal_system": [res.crystal_system[0], res.crystal_system[-1]], "n_translations": [res.n_translations[0], res.n_translations[-1]]}
ms, runs = timed(lambda: conventional_cell(lats, poss, zs, symprec=args.symprec, sym=sym))
lines.append({"what": "conventional_cell, all structures in one call, sym passed in", "ms": round(ms, 3), "ms_runs": runs, **what})
msp, runsp = timed(lambda: primitive_cell(lats, poss, zs, symprec=args.symprec, sym=sym))
lines.append({"what": "primitive_cell, all structures in one call, sym passed in", "ms": round(msp, 3), "ms_runs": runsp})
msf, runsf = timed(lambda: conventional_cell(lats, poss, zs, symprec=args.symprec))
lines.append({"what": "conventional_cell, all structures in one call, the symmetry search included", "ms": round(msf, 3), "ms_runs": runsf})
if not args.skip_single:
    syms = [find_symmetry(lats[b:b + 1], poss[b:b + 1], zs[b:b + 1], symprec=args.symprec) for b in range(B)]

    def one_by_one():
        for b in range(B):
            conventional_cell(lats[b:b + 1], poss[b:b + 1], zs[b:b + 1], symprec=args.symprec, sym=syms[b])
    ms1, runs1 = timed(one_by_one)
    lines.append({"what": "conventional_cell, the same structures one per call, sym passed in", "ms": round(ms1, 3), "ms_runs": runs1,
                  "over_the_batched_call": round(ms1 / ms, 2)})

out = {"tool": "tools/cells_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "single_species": B // 2, "four_species": B - B // 2, "symprec": args.symprec}, "runs": lines}
for line in lines:
    print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
