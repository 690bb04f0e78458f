"""Local structure analysis (alignn_amd.local_order) timed per function on a synthetic trajectory, so no model is needed:
--structs B structures of --atoms atoms with two species, --frames frames of N(0, --noise A) displacements about an fcc lattice
(nearest neighbours at --spacing A; with 200 atoms a 4 x 4 x 4 supercell cut to 200 rows, so the rows next to the cut have fewer
neighbours); ``cna`` with the fixed cutoff --rcut and with the adaptive rule inside --search, ``bond_order`` with l = 4, 6 (with
and without the averaged forms), and beside them the existing ``steinhardt`` with l = 4, 6 on the same tensors and the same --rcut
as the yardstick: all four walk the same neighbour lists.

Per function: the median of --repeats calls timed with device events after a warm-up call, and the (frame, atom) shells per
second.  ``bond_order`` is also timed pass by pass (the two entry points of include/alignn_local.h over the same chunks).  Writes
one JSON file (default profiles/local_time.json) and prints it.  All in one process."""
import argparse, ctypes as C, itertools, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alignn_amd import _lib, bond_order, cna, local_order, steinhardt

ap = argparse.ArgumentParser()
ap.add_argument("--structs", type=int, default=16)
ap.add_argument("--atoms", type=int, default=200)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--spacing", type=float, default=2.55)
ap.add_argument("--noise", type=float, default=0.08)
ap.add_argument("--rcut", type=float, default=3.08)
ap.add_argument("--search", type=float, default=3.9)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("local_time: no GPU; nothing is measured without one")
dev = "cuda"
B, n, F = args.structs, args.atoms, args.frames
rng = np.random.default_rng(7)
a = args.spacing * np.sqrt(2.0)
reps = int(np.ceil((n / 4) ** (1 / 3)))
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
grid = (np.array(list(itertools.product(range(reps), repeat=3)), dtype=np.float64)[:, None, :] + base[None]).reshape(-1, 3)[:n] * a
cell = np.eye(3) * reps * a
pos = torch.tensor(np.tile(grid, (B, 1))[None] + rng.normal(0.0, args.noise, (F, B * n, 3)), device=dev)
species = [np.where(np.arange(n) % 2 == 0, 13, 28) for _ in range(B)]
cells = torch.tensor(np.tile(cell[None], (B, 1, 1)), device=dev)
ns = [n] * B


def timed(fn, repeats=args.repeats):
    """Median (and all) of ``repeats`` calls in ms by device events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), [round(m, 3) for m in ms]


shells = F * B * n
lines = []


def line(what, fn, **more):
    ms, runs = timed(fn)
    lines.append({"what": what, "ms": round(ms, 3), "ms_runs": runs, "shells_per_s": round(shells / (ms * 1e-3), 1), **more})
    print(json.dumps(lines[-1]), flush=True)


st = steinhardt(pos, cells, ns, species, r_cut=args.rcut, ls=(4, 6))
fixed = cna(pos, cells, ns, species, r_cut=args.rcut)
adaptive = cna(pos, cells, ns, species, r_cut=args.search, adaptive=True)
nb = st.n_neighbors.double()
classes = lambda r: {name: round(float(r.fraction[:, 0, :, k].mean().item()), 4) for k, name in enumerate(local_order.CLASSES)}
line("steinhardt q4, q6 (the yardstick: triplet walk + means + the status word's read-back)", lambda: steinhardt(
    pos, cells, ns, species, r_cut=args.rcut, ls=(4, 6)), neighbors_mean=round(float(nb.mean().item()), 2), neighbors_at_most=int(nb.max().item()))
line("cna, fixed cutoff (signatures + counts + the status word's read-back)", lambda: cna(pos, cells, ns, species, r_cut=args.rcut),
     fractions=classes(fixed))
line("cna, adaptive (sort + one or two stages + counts + the read-back)", lambda: cna(pos, cells, ns, species, r_cut=args.search, adaptive=True),
     fractions=classes(adaptive), neighbors_mean=round(float(adaptive.n_neighbors.double().mean().item()), 2),
     neighbors_at_most=int(adaptive.n_neighbors.max().item()))
line("bond_order l = 4, 6 with the averaged forms (two passes per chunk + four means + the read-back)", lambda: bond_order(
    pos, cells, ns, species, r_cut=args.rcut, ls=(4, 6)))
line("bond_order l = 4, 6, average=False (pass 2 builds no list)", lambda: bond_order(pos, cells, ns, species, r_cut=args.rcut, ls=(4, 6),
                                                                                        average=False))

# pass by pass: the two entry points over the chunks bond_order would take
bo = bond_order(pos, cells, ns, species, r_cut=args.rcut, ls=(4, 6))
L, N = 2, B * n
lib = local_order._load()
from alignn_amd._trajectory_inputs import _groups
ptr, group, count, S, _ = _groups("local_time", ns, species, pos.device)
cut = torch.full((B,), args.rcut, dtype=torch.float64, device=dev)
table = np.zeros((L, local_order.W3J_STRIDE))
for u, l in enumerate((4, 6)):
    table[u, :(2 * l + 1) ** 2] = local_order.wigner_3j_table(l).reshape(-1)
w3j, ynorm = torch.tensor(table, device=dev), torch.tensor(np.array(local_order.ylm_norms()), device=dev)
chunk = max(1, min(F, local_order.QLM_SCRATCH_BYTES // (N * L * local_order.M_STRIDE * 16)))
qlm = torch.empty(chunk, N, L, local_order.M_STRIDE, 2, dtype=torch.float64, device=dev)
outs = {k: torch.zeros(F, N, L, dtype=torch.float64, device=dev) for k in ("s", "t", "q", "w", "s_avg", "t_avg", "q_avg", "w_avg")}
nn, status = torch.zeros(F, N, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
bargs = local_order.BondArgs(traj=pos.data_ptr(), lattice=cells.data_ptr(), atom_ptr=ptr.data_ptr(), group=group.data_ptr(),
                             group_count=count.data_ptr(), r_cut=cut.data_ptr(), ynorm=ynorm.data_ptr(), w3j=w3j.data_ptr(),
                             qlm=qlm.data_ptr(), n_neighbors=nn.data_ptr(), status=status.data_ptr(), n_structs=B, n_atoms=N, max_atoms=n,
                             n_species=S, n_total_frames=F, frame0=0, frame_step=1, n_frames=F, lattice_per_frame=0, average=1, n_ls=L,
                             l0=4, l1=6, **{k: v.data_ptr() for k, v in outs.items()})


def passes(entry):
    for chunk0 in range(0, F, chunk):
        bargs.chunk0, bargs.chunk_frames = chunk0, min(chunk, F - chunk0)
        _lib.check(entry(C.byref(bargs), _lib.stream()), "local_time")


line(f"bond_order pass 1 alone (lists + harmonics, {-(-F // chunk)} chunks of {chunk} frames)", lambda: passes(lib.alignn_local_bond_qlm))
line("bond_order pass 2 alone (lists again + gather + invariants; it reads pass 1's q_lm of the last chunk only: the same work)",
     lambda: passes(lib.alignn_local_bond_finish))
assert int(status.item()) == 0

out = {"tool": "tools/local_time.py", "device": torch.cuda.get_device_name(0),
       "workload": {"structs": B, "atoms": n, "species": 2, "frames": F, "spacing_A": args.spacing, "noise_A": args.noise,
                    "r_cut": args.rcut, "search_radius": args.search, "cell_A": reps * a, "qlm_chunk_frames": chunk},
       "repeats": args.repeats, "runs": lines}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
