"""The symmetry search (alignn_amd.symmetry.find_symmetry) timed on --structs structures of about 200 atoms, no model needed.
One half has a single species - 5 x 5 x 4 supercells of hcp, 200 atoms, 2400 operations each: every atom is a candidate for the
image of the pivot atom and every candidate is accepted, so the acceptance test runs to its end everywhere, the worst case.  The
other half is the same 200 sites decorated at random with 4 species: no symmetry beyond the identity, the candidates are the
atoms of the rarest species and most leave at their first 64 atoms.  The lattice constants differ from structure to structure.

Per measurement the median of --repeats calls timed with device events after a warm-up call: the whole call (the read-back of
the counts and the allocation of the results included), its two entry points apart (the search: lattice operations, acceptance,
summary; the fill: maps, shifts, orbits), the same structures searched one per call, and the three symmetrisers.  Writes one JSON
file (default profiles/sym_time.json) and prints it.  All in one process.  The share of the acceptance kernel inside the search
is a kernel-trace figure (rocprofv3 --kernel-trace --stats, a run of its own with --repeats 1 --skip-single)."""
import argparse, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import find_symmetry, symmetrize_forces, symmetrize_positions, symmetrize_stress
from alignn_amd import symmetry
from tests import sym_ref

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--symprec", type=float, default=1e-3)
ap.add_argument("--skip-single", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sym_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sym_time: no GPU; nothing is measured without one")
B = args.structs
rng = np.random.default_rng(7)
lats, poss, zs = [], [], []
for b in range(B):
    a = 3.2 * (1.0 + 0.002 * b)
    A, pos, z = sym_ref.supercell(sym_ref.hexagonal_cell(a, 1.633 * a), np.array([[1 / 3, 2 / 3, 0.25], [2 / 3, 1 / 3, 0.75]]) @ sym_ref.hexagonal_cell(a, 1.633 * a),
                                  np.array([12, 12]), (5, 5, 4))
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
res = find_symmetry(lats, poss, zs, symprec=args.symprec)
ops = sum(res.n_ops)
ms, runs = timed(lambda: find_symmetry(lats, poss, zs, symprec=args.symprec))
lines.append({"what": "find_symmetry, all structures in one call (read-back and allocation included)", "ms": round(ms, 3), "ms_runs": runs,
              "operations_found": ops, "single_species_operations_each": res.n_ops[0], "four_species_operations_each": res.n_ops[-1]})

# the two entry points apart: device events around each, inside the same calls
lib = symmetry._load()
stage_ms = {"alignn_sym_search": [], "alignn_sym_fill": []}
marks = []
originals = {name: getattr(lib, name) for name in stage_ms}
for name in stage_ms:
    def wrapped(*a, _fn=originals[name], _name=name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = _fn(*a)
        e1.record()
        marks.append((_name, e0, e1))
        return rc
    setattr(lib, name, wrapped)
for _ in range(args.repeats):
    find_symmetry(lats, poss, zs, symprec=args.symprec)
torch.cuda.synchronize()
for name, e0, e1 in marks:
    stage_ms[name].append(e0.elapsed_time(e1))
for name, fn in originals.items():
    setattr(lib, name, fn)
for name, what in (("alignn_sym_search", "the search alone: lattice operations, acceptance, summary"),
                   ("alignn_sym_fill", "the fill alone: rotations, translations, atom maps, shifts, orbits")):
    lines.append({"what": what, "ms": round(statistics.median(stage_ms[name]), 3), "ms_runs": [round(m, 3) for m in stage_ms[name]]})

if not args.skip_single:
    def one_by_one():
        for b in range(B):
            find_symmetry(lats[b:b + 1], poss[b:b + 1], zs[b:b + 1], symprec=args.symprec)
    ms1, runs1 = timed(one_by_one)
    lines.append({"what": "the same structures, one per call", "ms": round(ms1, 3), "ms_runs": runs1, "over_the_batched_call": round(ms1 / ms, 2)})
    for half, sl in (("single species", slice(0, B // 2)), ("four species", slice(B // 2, B))):
        msh, runsh = timed(lambda: find_symmetry(lats[sl], poss[sl], zs[sl], symprec=args.symprec))
        lines.append({"what": f"the {half} half alone, one call", "ms": round(msh, 3), "ms_runs": runsh})

F = torch.tensor(rng.normal(size=(B * n, 3)), device="cuda")
S = torch.tensor(rng.normal(size=(B, 3, 3)), device="cuda")
P = torch.tensor(np.concatenate(poss), device="cuda")
L = torch.tensor(np.array(lats), device="cuda")
for name, fn in (("symmetrize_forces", lambda: symmetrize_forces(res, L, F)), ("symmetrize_stress", lambda: symmetrize_stress(res, L, S)),
                 ("symmetrize_positions", lambda: symmetrize_positions(res, L, P))):
    msx, runsx = timed(fn)
    lines.append({"what": name, "ms": round(msx, 3), "ms_runs": runsx, "terms": ops * (9 if name.endswith("stress") else n)})

out = {"tool": "tools/sym_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "single_species": B // 2, "four_species": B - B // 2, "symprec": args.symprec}, "runs": lines}
for line in lines:
    print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
