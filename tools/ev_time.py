"""The E-V curve task (alignn_amd.eos) timed: --batch crystals of --atoms atoms (synthetic.make_crystal) x the reference's ten
strains, the tools/relax_time.py model.  Batched: one ev_curve call.  Reference shape: one evaluation call (relax, steps = 0) per
strained structure and one host fit per crystal (tests/eos_ref.py ase_fit: ASE's two scipy curve_fit calls), as the reference's
loop runs (alignn/ff/ff.py:762-805), on the structures the batched call built.  A random model's curve need not have a minimum:
host fits that scipy gives up on are counted, not fatal.  The fit launch is also timed alone (events around --fit-repeats
launches), on the call's own curves and on --fit-structures noisy Murnaghan curves.  Informational; prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, eos_fit, ev_curve, relax
from alignn_amd.synthetic import make_crystal
from tests import eos_ref

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--atoms", type=int, default=8)
ap.add_argument("--eos", default="murnaghan")
ap.add_argument("--fit-structures", type=int, default=4096)
ap.add_argument("--fit-repeats", type=int, default=20)
args = ap.parse_args()
dev = "cuda"
torch.manual_seed(0)
model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                             atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
B, dx = args.batch, np.arange(-0.05, 0.05, 0.01)
lats, pos, feats = [], [], []
for i in range(B):
    lat, frac, _ = make_crystal(args.atoms, 4321 + i)
    lats.append(np.asarray(lat, dtype=np.float64))
    pos.append(np.asarray(frac, dtype=np.float64) @ lats[-1])
    feats.append(torch.randn(args.atoms, 92, device=dev))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_by_one(n):
    """The reference's loop over the first n crystals -> (evaluation calls, host fits that failed)."""
    calls = failed = 0
    for s in range(n):
        vol, en = [], []
        for d in dx:
            cell, cart, v = eos_ref.strain(lats[s], pos[s], eos_ref.isotropic(d))
            en.append(float(relax(model, [cell], [cart], [feats[s]], steps=0).energies[0]))
            vol.append(v)
            calls += 1
        try:
            eos_ref.ase_fit(vol, en, eos_ref.FORMS[args.eos])
        except (RuntimeError, ValueError, FloatingPointError):
            failed += 1
    return calls, failed


def fit_alone(vol, en):
    """Median time of one fit launch (s), events around each of --fit-repeats launches after a warm-up."""
    eos_fit(vol, en, args.eos)
    times = []
    for _ in range(args.fit_repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eos_fit(vol, en, args.eos)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


call = lambda: ev_curve(model, lats, pos, feats, dx=dx, eos=args.eos)
call()  # the warm-up of this batch's shapes
t_b, res = timed(call)
one_by_one(1)  # warm-up
t_1, (calls, failed) = timed(lambda: one_by_one(B))
t_fit_own = fit_alone(torch.tensor(res.volumes, device=dev), torch.tensor(res.energies, device=dev))
rng = np.random.default_rng(0)
N = args.fit_structures
v0 = rng.uniform(40.0, 120.0, N)
V = v0[:, None] * (1.0 + dx[None, :]) ** 3
E = np.stack([eos_ref.ASE_FORMS[eos_ref.FORMS[args.eos]](V[i], -3.2, 0.6, 4.5, 1.015 * v0[i]) for i in range(N)])
E = E + rng.normal(0.0, 1e-4, E.shape)
Vd, Ed = torch.tensor(V, device=dev), torch.tensor(E, device=dev)
t_fit_many = fit_alone(Vd, Ed)
params, rms, n_iter, status = eos_fit(Vd, Ed, args.eos)
t0 = time.perf_counter()
n_host = min(N, 64)
for i in range(n_host):
    eos_ref.ase_fit(V[i], E[i], eos_ref.FORMS[args.eos])
t_host_fit = (time.perf_counter() - t0) / n_host
print(json.dumps({"task": "ev_curve", "B": B, "atoms": args.atoms, "K": len(dx), "eos": args.eos, "structures": B * len(dx),
                  "eval_calls": res.n_eval_calls, "batched_s": round(t_b, 4), "status": res.status.tolist(),
                  "reference_shape_eval_calls": calls, "reference_shape_host_fits_failed": failed,
                  "reference_shape_s": round(t_1, 4), "speedup": round(t_1 / t_b, 2),
                  "fit_launch_us_own_curves": round(t_fit_own * 1e6, 1), "fit_structures": N,
                  "fit_launch_us": round(t_fit_many * 1e6, 1), "fit_ns_per_structure": round(t_fit_many / N * 1e9, 1),
                  "fit_steps_mean": round(float(n_iter.double().mean()), 2), "fit_converged": int((status == 0).sum()),
                  "host_scipy_fit_us_per_structure": round(t_host_fit * 1e6, 1)}), flush=True)
