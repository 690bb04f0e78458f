"""The IDPP band initialisation (alignn_amd.idpp) timed: --bands bands of --images interior images of --atoms atoms
(synthetic.make_crystal, the final image the initial one with every atom displaced by a random 0.3 A), float64 throughout.
Three things, each the median of --repeats runs with their spread: (1) one ``alignn_idpp_forces`` launch on the straight path, by
device events over --launches launches; (2) one FIRE step of the pass (``idpp_interpolate`` with fmax = 0, so every band takes
exactly --steps steps: the launch, ``alignn_neb_forces``, ``alignn_fire_step`` and the step's host read); (3) the same objective
as a float64 torch expression over dense [images, n, n] tensors on the same GPU.  Writes one JSON file (default
profiles/idpp_time.json) and prints it."""
import argparse, ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import _lib, idpp_interpolate, neb_interpolate
from alignn_amd.idpp import IdppArgs, _load
from alignn_amd.synthetic import make_crystal

ap = argparse.ArgumentParser()
ap.add_argument("--bands", type=int, default=16)
ap.add_argument("--atoms", type=int, default=200)
ap.add_argument("--images", type=int, default=7, help="interior images per band")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "idpp_time.json"))
args = ap.parse_args()
dev = "cuda"
B, n, I = args.bands, args.atoms, args.images
rng = np.random.default_rng(0)
lats, first, last = [], [], []
for i in range(B):
    lat, frac, _ = make_crystal(n, 4321 + i)
    p = np.asarray(frac @ lat, dtype=np.float64)
    lats.append(np.asarray(lat, dtype=np.float64))
    first.append(p)
    last.append(p + rng.normal(0.0, 0.3 / np.sqrt(3.0), p.shape))
t64 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64, device=dev)
lat_t, first_t, last_t = t64(np.stack(lats)), t64(np.concatenate(first)), t64(np.concatenate(last))
rows, inv = neb_interpolate(lat_t, first_t, last_t, [n] * B, [I + 2] * B)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "runs": [round(x, 4) for x in xs]}


# --- (1) the launch ----------------------------------------------------------------------------------------------------------------
pre = lambda c: torch.tensor(np.concatenate([[0], np.cumsum(c)]), dtype=torch.int32, device=dev)
keep = dict(force_ptr=pre([I * n] * B), energy_ptr=pre([I] * B), active=torch.arange(B, dtype=torch.int32, device=dev),
            row_ptr=pre([I * n] * B), end_ptr=pre([n] * B), lattice=lat_t, inv_lattice=inv, initial=first_t, final=last_t,
            positions=rows, forces=torch.empty_like(rows), energy=torch.empty(B * I, dtype=torch.float64, device=dev),
            row_energy=torch.empty(B * I * n, dtype=torch.float64, device=dev),
            status=torch.empty(B, dtype=torch.int32, device=dev))
block = IdppArgs(n_active=B, max_images=I + 2, max_atoms=n, **{k: v.data_ptr() for k, v in keep.items()})
lib = _load()


def launches():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        _lib.check(lib.alignn_idpp_forces(C.byref(block), _lib.stream()), "idpp_forces")
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.launches  # ms per launch


launches()  # warm-up: the code object
t_launch = [launches() for _ in range(args.repeats)]
assert keep["status"].eq(0).all()


# --- (2) a FIRE step of the pass ------------------------------------------------------------------------------------------------------
def the_pass():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = idpp_interpolate(lats, first, last, n_images=I, fmax=0.0, steps=args.steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / res.n_evals, res


the_pass()
runs = [the_pass() for _ in range(args.repeats)]
t_step, res = [r[0] for r in runs], runs[0][1]


# --- (3) the objective as a torch expression ---------------------------------------------------------------------------------------------
def wrapped(R, Cm, Ci):
    """|mic(R_a - R_b)| and the wrapped differences of [K, n, 3] images in the cells Cm [K, 3, 3]."""
    d = R[:, :, None, :] - R[:, None, :, :]
    f = torch.einsum("kabi,kij->kabj", d, Ci)
    D = torch.einsum("kabi,kij->kabj", f - torch.round(f), Cm)
    return D, torch.sqrt((D * D).sum(-1))


cells = lat_t.repeat_interleave(I, 0)
invs = inv.repeat_interleave(I, 0)
m = torch.arange(1, I + 1, dtype=torch.float64, device=dev).repeat(B)[:, None, None]
off = ~torch.eye(n, dtype=torch.bool, device=dev)[None]


def torch_objective():
    R = rows.view(B * I, n, 3)
    d1 = wrapped(first_t.view(B, n, 3), lat_t, inv)[1].repeat_interleave(I, 0)
    d2 = wrapped(last_t.view(B, n, 3), lat_t, inv)[1].repeat_interleave(I, 0)
    D, d = wrapped(R, cells, invs)
    delta = d - (d1 + m * ((d2 - d1) / (I + 1)))
    d4 = (d * d) ** 2
    e = torch.where(off, delta * delta / d4, torch.zeros_like(d))
    c = torch.where(off, delta * (1.0 - 2.0 * delta / d) / (d4 * d), torch.zeros_like(d))
    return 0.5 * e.sum((1, 2)), -2.0 * (c[..., None] * D).sum(2)


def torch_runs():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        torch_objective()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 5


E_t, F_t = torch_objective()
err_f = float((F_t.reshape(-1, 3) - keep["forces"]).abs().max() / keep["forces"].abs().max())
err_e = float(((E_t - keep["energy"]).abs() / keep["energy"].abs()).max())
t_torch = [torch_runs() for _ in range(args.repeats)]

out = {"tool": "tools/idpp_time.py", "device": torch.cuda.get_device_name(0), "bands": B, "atoms": n, "interior_images": I,
       "ordered_pairs_per_launch": B * I * n * (n - 1), "idpp_forces_launch_ms": spread(t_launch),
       "pass_ms_per_fire_step": spread(t_step), "pass_steps": int(res.n_steps[0]), "pass_evaluations": res.n_evals,
       "torch_float64_objective_ms": spread(t_torch), "torch_over_launch": round(statistics.median(t_torch) / statistics.median(t_launch), 1),
       "kernel_vs_torch_max_rel_force_difference": err_f, "kernel_vs_torch_max_rel_energy_difference": err_e}
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
