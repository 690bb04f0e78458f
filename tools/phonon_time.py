"""Batched phonons (alignn_amd.phonons) timed: B in {1, 8, 32} crystals of 4 and 8 atoms (synthetic.make_crystal), supercell
(3, 3, 3), the tools/md_step.py model, a 100-point q-path and the 20^3 DOS mesh.  Beside each batch, the reference's shape:
one displaced supercell per model call, then host numpy D(q) + eigvalsh over the same q-path and mesh, structure after
structure (timed on the first --ref-structures structures and scaled to B: the loop is sequential in B).  --eigh: the eigen
launch alone against host numpy eigvalsh for K q-points and m in {12, 24, 48, 96}.  --chunks: time and peak memory of
phonons() per max_atoms_per_eval.  --displacements all|symmetry|all,symmetry: diamond, rocksalt and wurtzite (built here: the
random cells have no symmetry) at (3, 3, 3), each alone and the three together, with every atom displaced along x, y, z and / or
with the symmetry-reduced displacements (find_symmetry timed apart); both modes in one invocation put the supercell counts and
times side by side.  Prints one JSON line per measurement."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, find_symmetry, neighbors, phonons
from alignn_amd.phonons import FREQ_SCALE, _eigh, lattice_points, monkhorst_pack
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8,32")
ap.add_argument("--atoms", default="4,8")
ap.add_argument("--ref-structures", type=int, default=1)
ap.add_argument("--eigh", action="store_true")
ap.add_argument("--eigh-k", type=int, default=8000)
ap.add_argument("--eigh-host-k", type=int, default=500)
ap.add_argument("--chunks", default="")
ap.add_argument("--skip-batches", action="store_true")
ap.add_argument("--displacements", default="", help="all, symmetry or all,symmetry: time the symmetric crystals")
args = ap.parse_args()
dev = "cuda"
SC = (3, 3, 3)
QPATH = np.stack([np.linspace(0, 0.5, 100), np.linspace(0, 0.25, 100), np.zeros(100)], 1)
MESH = monkhorst_pack((20, 20, 20))


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def structures(B, n):
    lats, pos, feats, masses = [], [], [], []
    for i in range(B):
        lat, frac, _ = make_crystal(n, 7000 + 97 * n + i)
        lats.append(np.asarray(lat, dtype=np.float64))
        pos.append(np.asarray(frac, dtype=np.float64) @ lats[-1])
        feats.append(torch.randn(n, 92, device=dev))
        masses.append(np.random.default_rng(i).uniform(10.0, 100.0, n))
    return lats, pos, feats, masses


def host_dispersion(C, m, qs):
    """The reference's band_structure on the host: D(q) = sum_R D_R exp(-2 pi i q.R), eigvalsh, q after q."""
    w = np.repeat(np.asarray(m) ** -0.5, 3)
    D_N = C * np.outer(w, w)[None]
    R = lattice_points(SC)
    out = []
    for q in qs:
        Dq = np.sum(np.exp(-2j * np.pi * (R @ q))[:, None, None] * D_N, axis=0)
        out.append(np.linalg.eigvalsh(Dq, UPLO="U"))
    return out


def reference_loop(model, lats, pos, feats, masses, delta=0.01):
    """One displaced supercell per model call, force constants in numpy, then the host dispersion."""
    from tests.phonons_ref import displaced_supercells, force_constants, inv_supercell

    for lat, p, f, m in zip(lats, pos, feats, masses):
        n = len(p)
        sl = torch.tensor(lat * np.array(SC, dtype=np.float64)[:, None], device=dev)
        f_sc = f.repeat(27, 1)
        forces = []
        for fr, _ in displaced_supercells(lat, p, SC, delta, inv_supercell(lat, SC)):
            batch = neighbors.crystal_batch([sl], [torch.tensor(fr, device=dev)], atom_features=[f_sc], device=dev)
            with torch.enable_grad():
                out = model(batch)
            forces.append(out["grad"].detach().reshape(-1, 3).double().cpu().numpy())
        C = force_constants(forces, n, SC, delta)
        host_dispersion(C, m, QPATH)
        host_dispersion(C, m, MESH)


torch.manual_seed(0)
model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                             atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
kw = dict(supercell=SC, delta=0.01, qpoints=QPATH, dos_kpts=(20, 20, 20), dos_npts=100, dos_width=1e-3)

if args.chunks:
    lats, pos, feats, masses = structures(8, 8)
    phonons(model, lats[:1], pos[:1], feats[:1], masses[:1], **{**kw, "dos_kpts": None})  # warm-up
    for c in [int(x) for x in args.chunks.split(",")]:
        phonons(model, lats, pos, feats, masses, max_atoms_per_eval=c, **{**kw, "dos_kpts": None})
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t, res = sync_time(lambda: phonons(model, lats, pos, feats, masses, max_atoms_per_eval=c, **{**kw, "dos_kpts": None}))
        print(json.dumps({"what": "chunk", "max_atoms_per_eval": c, "B": 8, "atoms": 8, "supercell": SC, "n_evals": res.n_evals,
                          "s": round(t, 3), "peak_workspace_GiB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)}),
              flush=True)



def symmetric_crystals():
    """name -> (cell, Cartesian positions, species, masses): diamond and rocksalt on the fcc primitive cell, wurtzite."""
    fcc = lambda a: 0.5 * a * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    hexa = lambda a, c: np.array([[a, 0.0, 0.0], [-0.5 * a, 0.5 * np.sqrt(3.0) * a, 0.0], [0.0, 0.0, c]])
    raw = {"diamond": (fcc(3.57), [[0, 0, 0], [0.25, 0.25, 0.25]], [6, 6], [12.011, 12.011]),
           "rocksalt": (fcc(5.64), [[0, 0, 0], [0.5, 0.5, 0.5]], [11, 17], [22.99, 35.45]),
           "wurtzite": (hexa(3.25, 5.21), [[1 / 3, 2 / 3, 0.0], [2 / 3, 1 / 3, 0.5], [1 / 3, 2 / 3, 0.382], [2 / 3, 1 / 3, 0.882]],
                        [30, 30, 8, 8], [65.38, 65.38, 15.999, 15.999])}
    return {k: (A, np.asarray(f, dtype=np.float64) @ A, np.asarray(z), np.asarray(m)) for k, (A, f, z, m) in raw.items()}


if args.displacements:
    modes = args.displacements.split(",")
    if any(m not in ("all", "symmetry") for m in modes):
        ap.error("--displacements takes all, symmetry or all,symmetry")
    crystals = symmetric_crystals()
    g = torch.Generator(device="cpu").manual_seed(1)
    kinds = {z: torch.randn(92, generator=g).to(dev) for z in (6, 11, 17, 30, 8)}
    groups = [[k] for k in crystals] + [list(crystals)]
    for names in groups:
        lats, pos, zs, masses = ([crystals[k][i] for k in names] for i in range(4))
        feats = [torch.stack([kinds[int(v)] for v in z]) for z in zs]
        find_symmetry(lats, pos, zs)  # warm-up
        t_sym, sym = sync_time(lambda: find_symmetry(lats, pos, zs))
        for mode in modes:
            extra = dict(displacements="symmetry", symmetry=sym) if mode == "symmetry" else {}
            no_q = {**kw, "qpoints": None, "dos_kpts": None, **extra}
            phonons(model, lats, pos, feats, masses, **{**kw, **extra})  # warm-up
            t_all, res = sync_time(lambda: phonons(model, lats, pos, feats, masses, **{**kw, **extra}))
            t_fc, _ = sync_time(lambda: phonons(model, lats, pos, feats, masses, **no_q))
            print(json.dumps({"what": "displacements", "crystals": "+".join(names), "mode": mode, "supercell": SC,
                              "supercells": res.n_supercells, "n_evals": res.n_evals, "force_constants_s": round(t_fc, 4),
                              "with_q_path_and_dos_s": round(t_all, 4),
                              "find_symmetry_s": round(t_sym, 4) if mode == "symmetry" else None}), flush=True)

if not args.skip_batches:
    for n in [int(x) for x in args.atoms.split(",")]:
        lats, pos, feats, masses = structures(max(int(b) for b in args.batches.split(",")), n)
        phonons(model, lats[:2], pos[:2], feats[:2], masses[:2], **kw)  # warm-up: code objects, allocator
        nr = args.ref_structures
        reference_loop(model, lats[:1], pos[:1], feats[:1], masses[:1])  # warm-up
        t_ref, _ = sync_time(lambda: reference_loop(model, lats[:nr], pos[:nr], feats[:nr], masses[:nr]))
        for B in [int(b) for b in args.batches.split(",")]:
            phonons(model, lats[:B], pos[:B], feats[:B], masses[:B], **kw)
            t_b, res = sync_time(lambda: phonons(model, lats[:B], pos[:B], feats[:B], masses[:B], **kw))
            t_r = t_ref / nr * B
            print(json.dumps({"what": "phonons", "B": B, "atoms": n, "supercell": SC, "supercells": res.n_supercells,
                              "n_evals": res.n_evals, "q_path": len(QPATH), "dos_mesh": len(MESH), "batched_s": round(t_b, 3),
                              "reference_shape_s": round(t_r, 3), "reference_structures_timed": nr, "speedup": round(t_r / t_b, 1)}),
                  flush=True)

if args.eigh:
    rng = np.random.default_rng(0)
    K = args.eigh_k
    q = rng.uniform(-0.5, 0.5, (K, 3))
    R = lattice_points(SC)
    for m in (12, 24, 48, 96):
        A = rng.normal(size=(27, m, m)) * np.exp(-np.abs(R).sum(1))[:, None, None]
        D_N = 0.5 * (A + A[[list(map(tuple, R)).index(tuple(-r)) for r in R]].transpose(0, 2, 1))
        state = dict(device=torch.device(dev), m=[m], dyn=torch.tensor(D_N.reshape(-1), device=dev),
                     off=torch.zeros(1, dtype=torch.int64, device=dev), R=torch.tensor(R, dtype=torch.int32, device=dev),
                     cell_ptr=torch.tensor([0, 27], dtype=torch.int32, device=dev), dims=torch.tensor([m], dtype=torch.int32, device=dev))
        _eigh(state, q[:64], False)
        t_dev, (f, _) = sync_time(lambda: _eigh(state, q, False))
        t_dev_modes, _ = sync_time(lambda: _eigh(state, q, True))
        kh = min(K, args.eigh_host_k)
        t0 = time.perf_counter()
        ev = np.array([np.linalg.eigvalsh(np.sum(np.exp(-2j * np.pi * (R @ qq))[:, None, None] * D_N, axis=0), UPLO="U")
                       for qq in q[:kh]])
        t_host = (time.perf_counter() - t0) / kh * K
        w = np.sign(ev) * FREQ_SCALE * np.sqrt(np.abs(ev))
        err = np.abs(f[0].cpu().numpy()[:kh] - w).max() / np.abs(w).max()
        print(json.dumps({"what": "eigh", "K": K, "m": m, "device_ms": round(1e3 * t_dev, 3),
                          "device_modes_ms": round(1e3 * t_dev_modes, 3), "host_ms": round(1e3 * t_host, 1),
                          "host_q_timed": kh, "speedup": round(t_host / t_dev, 1), "max_rel_diff": float(f"{err:.2e}")}),
              flush=True)
