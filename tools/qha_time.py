"""The quasi-harmonic task (alignn_amd.thermo) timed.  (1) One qha call on --batch crystals of --atoms atoms
(synthetic.make_crystal), the tools/ev_time.py model, the reference's ten strains and 101 temperatures, by stage: the stages are
timed one after the other on the call's own structures (the E(V) evaluations, the one phonons call, the mesh frequencies, the
sums launch, the fit launch on B NT curves, the reduction), then the whole call.  (2) The sums launch alone against the same four
sums written as torch float64 expressions on the device, on a --mesh^3 mesh x --modes modes x 101 temperatures (events around
--repeats launches after a warm-up; the torch expressions go temperature by temperature, as a [NT, n] intermediate of 8e7
doubles per quantity would).  Recorded numbers, not a gate; prints one JSON line per measurement."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig, eos_fit, ev_curve, phonons, qha, thermal_properties, thermal_sums
from alignn_amd.phonons import monkhorst_pack
from alignn_amd.synthetic import make_crystal
from alignn_amd.thermo import KB, qha_derive
from tests import eos_ref

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--atoms", type=int, default=4)
ap.add_argument("--mesh", type=int, default=20)
ap.add_argument("--modes", type=int, default=96)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--skip-call", action="store_true")
args = ap.parse_args()
dev = "cuda"
T = np.arange(0.0, 1001.0, 10.0)
dx = np.arange(-0.05, 0.05, 0.01)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launch_time(fn):
    """Median time of one call of fn (s): events around each of --repeats calls after a warm-up."""
    fn()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


if not args.skip_call:
    torch.manual_seed(0)
    model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=4, gcn_layers=4, hidden_features=256,
                                                 atom_input_features=92, calculate_gradient=True, stresswise_weight=0.05)).to(dev).eval()
    B, P, NT = args.batch, len(dx), len(T)
    lats, pos, feats, masses = [], [], [], []
    for i in range(B):
        lat, frac, _ = make_crystal(args.atoms, 4321 + i)
        lats.append(np.asarray(lat, dtype=np.float64))
        pos.append(np.asarray(frac, dtype=np.float64) @ lats[-1])
        feats.append(torch.randn(args.atoms, 92, device=dev))
        masses.append(np.random.default_rng(i).uniform(10.0, 100.0, args.atoms))
    mesh = (args.mesh,) * 3
    call = lambda: qha(model, lats, pos, feats, masses, dx=dx, temperatures=T, mesh=mesh)
    call()  # the warm-up of this batch's shapes
    t_call, res = timed(call)
    # the stages, on the structures the call built
    t_ev, ev = timed(lambda: ev_curve(model, lats, pos, feats, dx=dx))
    built = [eos_ref.strain(lats[s], pos[s], eos_ref.isotropic(d)) for s in range(B) for d in dx]
    job = lambda x: [x[s] for s in range(B) for _ in dx]
    t_ph, ph = timed(lambda: phonons(model, [b[0] for b in built], [b[1] for b in built], job(feats), job(masses), qpoints=None,
                                     dos_kpts=None))
    q = np.ascontiguousarray(monkhorst_pack(mesh))
    t_mesh, fr = timed(lambda: ph.frequencies_at(q))
    flat = torch.cat([f.reshape(-1) for f in fr])
    off = np.concatenate([[0], np.cumsum([f.numel() for f in fr])])
    t_sums = launch_time(lambda: thermal_sums(flat, off, len(q), T))
    F, U, S, Cv, zpe, skipped = thermal_sums(flat, off, len(q), T)
    vol, en = torch.tensor(res.volumes, device=dev), torch.tensor(res.energies, device=dev)
    vol_rows = vol[:, None, :].expand(B, NT, P).reshape(B * NT, P)
    en_rows = (en[:, None, :] + F.view(B, P, NT).transpose(1, 2)).reshape(B * NT, P)
    t_fit = launch_time(lambda: eos_fit(vol_rows, en_rows))
    params, _, _, status = eos_fit(vol_rows, en_rows)
    params, T_d = params.view(B, NT, 4), torch.tensor(T, device=dev)
    derive = lambda: qha_derive(vol, Cv.view(B, P, NT), S.view(B, P, NT), T_d, params[..., 3].contiguous(),
                                params[..., 1].contiguous(), status.view(B, NT))
    t_derive = launch_time(derive)
    print(json.dumps({"task": "qha", "B": B, "atoms": args.atoms, "P": P, "NT": NT, "mesh": mesh, "structures": B * P,
                      "eval_calls": res.n_eval_calls, "phonon_evals": res.n_phonon_evals, "call_s": round(t_call, 4),
                      "stage_ev_curve_s": round(t_ev, 4), "stage_phonons_s": round(t_ph, 4), "stage_mesh_eigh_s": round(t_mesh, 4),
                      "stage_sums_launch_ms": round(t_sums * 1e3, 3), "stage_fit_launch_ms": round(t_fit * 1e3, 3),
                      "stage_derive_launch_us": round(t_derive * 1e6, 1), "skipped_modes": int(res.n_skipped.sum()),
                      "fits_converged": int((res.fit_status == 0).sum()), "inside": int(res.inside.sum())}), flush=True)

# the sums launch against torch float64 expressions
n_q, m = args.mesh ** 3, args.modes
freqs = torch.tensor(np.random.default_rng(0).uniform(1e-3, 0.08, n_q * m), device=dev)
off = np.array([0, n_q * m])
T_d = torch.tensor(T, device=dev)


def torch_sums():
    eps = freqs[freqs > 0.0]
    out = torch.empty(4, len(T), dtype=torch.float64, device=dev)
    for i in range(len(T)):
        if T[i] == 0.0:
            out[:2, i], out[2:, i] = 0.5 * eps.sum() / n_q, 0.0
            continue
        kT = KB * T[i]
        x = eps / kT
        em, om = torch.exp(-x), -torch.expm1(-x)
        lg = torch.log(om)
        out[0, i] = (0.5 * eps + kT * lg).sum() / n_q
        out[1, i] = (eps * (0.5 + em / om)).sum() / n_q
        out[2, i] = KB * (x * em / om - lg).sum() / n_q
        out[3, i] = KB * ((x / om) ** 2 * em).sum() / n_q
    return out


t_kernel = launch_time(lambda: thermal_sums(freqs, off, n_q, T))
t_torch = launch_time(torch_sums)
got, want = torch.stack(thermal_sums(freqs, off, n_q, T)[:4])[:, 0], torch_sums()
dev_rel = float(((got - want).abs().amax(1) / want.abs().amax(1)).max())
print(json.dumps({"task": "thermal_sums", "n_q": n_q, "modes": m, "NT": len(T), "terms": n_q * m * len(T),
                  "kernel_ms": round(t_kernel * 1e3, 3), "torch_float64_ms": round(t_torch * 1e3, 3),
                  "speedup": round(t_torch / t_kernel, 1), "kernel_ns_per_term": round(t_kernel / (n_q * m * len(T)) * 1e9, 4),
                  "max_rel_diff": float(f"{dev_rel:.2e}")}), flush=True)
