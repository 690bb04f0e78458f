"""The remaining workflow launches - the FIRE step and its cell filter, the seven MD ensembles, NEB and IDPP, the finite-displacement
phonon kernels, the defect, slab, strain and interface builders, the ZSL matcher, the EOS and elastic fits, the harmonic and
quasi-harmonic sums and the flat trajectory entry points - each between the guard bands of tests/gate_parity.py, every buffer of
exactly the extent its header states (tests/step_extents.py).  Asserted per launch, in this order: (a) no guard bit changed;
(b) the elements the header says the launch writes hold no pattern element, and those it says the launch leaves alone still hold
the pattern (``out`` arrays: the exact count) or the bits that were copied in (``state`` arrays) - which elements those are is
computed here on the host, from the inputs alone; (c) every ``out``, ``add`` and ``state`` array equals, bit for bit, what the
same entry point gives for the same inputs on plain allocations of the same extents, and the driver's result where one driver
call is exactly that launch (the headers promise bits that depend on a structure's own data alone, and the step-by-step modules
tie those bits to the numpy restatements); an input array is never changed.

The inputs are random and finite, physical sense is not needed; every one is an input whose behaviour the header defines.

Blind spots (those of the instrument): an access farther from a buffer than its guard - 1024 elements or two rows - and a read
beside a buffer whose value is never used."""

import numpy as np
import pytest
import torch

from alignn_amd import _abi, _lib, match_lattices, thermal_sums
from alignn_amd.dynamics import FS, KB
from alignn_amd.elastic import elastic_fit
from alignn_amd.eos import EOS_FORMS, eos_fit
from alignn_amd._jobs import build_slabs, strain_jobs
from alignn_amd._structures import pack
from alignn_amd.idpp import idpp_forces
from alignn_amd.interface import _plane_cell
from alignn_amd.neb import _inv3_cof, neb_interpolate
from alignn_amd.phonons import FREQ_SCALE, lattice_points, phonons
from alignn_amd.thermo import qha_derive
from alignn_amd.trajectory import green_kubo, vdos
from tests import defects_ref, elastic_ref, eos_ref, interface_ref
from tests import gate_parity as gp
from tests import step_extents as sx
from tests import workflow_extents as wx

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, I32, I64, U8 = torch.float64, torch.int32, torch.int64, torch.uint8


def _t(x, dtype=F64):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _library():
    lib = _lib.load()
    for name in ("alignn_neb.h", "alignn_idpp.h", "alignn_thermo.h", "alignn_traj.h"):
        _lib.bind(_abi.header(name), lib)
    return lib


def _report(case):
    return gp.Report(case, tag="step-extents")


def _block(rep, struct):
    return wx.Block(rep.guards, struct, DEV, rep.case, table=sx.STRUCTS)


def _call(rep, entry):
    return sx.Call(rep.guards, entry, DEV, rep.case)


def _eq(a, b):
    """the same bits in the same order (a guarded payload is [rows, row length], whatever shape the driver gives its array)"""
    return a.numel() == b.numel() and a.dtype == b.dtype and torch.equal(sx.bits(a).reshape(-1), sx.bits(b.contiguous()).reshape(-1))


def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _rows(ptr, which, width=1, skip=None):
    """[ptr[-1] * width] bool: the rows of the structures ``which`` (``skip``: a [ptr[-1]] bool array of rows to leave out)"""
    m = np.zeros(int(ptr[-1]), dtype=bool)
    for s in which:
        m[ptr[s]:ptr[s + 1]] = True
    if skip is not None:
        m &= ~np.asarray(skip, dtype=bool)
    return torch.tensor(np.repeat(m, width))


def _items(n, which, width=1):
    m = np.zeros(n, dtype=bool)
    m[list(which)] = True
    return torch.tensor(np.repeat(m, width))


def _launch(b, lib, plain, expect=0):
    """(a): the launch between the guards (``launch`` checks every guard of the registry), then the same on plain allocations"""
    if isinstance(b, sx.Call):
        b.launch(lib, _lib.stream(), expect=expect)
    else:
        b.launch(lib, b.table["entries"][0], _lib.stream())
    sx.plain_launch(b, lib, plain, _lib.stream(), expect=expect)


_verify = sx.verify  # (b) and (c); tests/test_workflow_extents.py plants each kind of finding and sees it reported


def _flat_case(rep, entry, scalars, inputs, null=(), written=None, expect=0):
    """one flat launch: allocate, (a), (b), (c) -> (the call, its payload)"""
    lib = _library()
    c = _call(rep, entry).set(**scalars).alloc(inputs, null)
    plain = sx.plain_copy(c)
    _launch(c, lib, plain, expect)
    _verify(c, plain, written)
    return c, c.payload


# ======================================================================================================================
# FIRE
# ======================================================================================================================
FIRE_NS = [1, 3, 257, 5]  # 257: one row past a 256-thread stride
FILTER = ("stress", "lattice0", "xa", "xc", "cell_velocities", "defgrad", "lattice", "stress_out")
OPTIONS = ("cell_mask", "scalar_pressure", "enthalpy_out")
PER_LAUNCH = ("forces", "energy", "stress", "force_ptr", "active", "status")


@pytest.mark.parametrize("cell,fixed,options", [(False, False, False), (False, True, False), (True, False, False), (True, True, True)])
def test_fire_step_between_guards(cell, fixed, options):
    """B = 4, active = [2, 0, 3] (out of order, structure 1 left out), steps = 2.  Launch 1: structure 0 has zero forces and
    converges, 2 and 3 step.  Launch 2: active = [2, 3], structure 3's force rows are 4 for its 5 atoms: status -1, nothing of
    it written; 2 steps.  Launch 3: 2 has taken its 2 steps and retires, 3 steps.  Nothing of structure 1 is ever written."""
    lib, rng = _library(), np.random.default_rng(17)
    ns, ptr = FIRE_NS, _ptr(FIRE_NS)
    B, N = len(ns), int(ptr[-1])
    rep = _report(f"fire cell={cell} fixed={fixed} options={options}")
    lat0 = 6.0 * np.eye(3) + 0.3 * rng.normal(size=(B, 3, 3))
    pos = rng.uniform(0.0, 6.0, (N, 3))
    fix = np.zeros(N, dtype=bool)
    fix[[ptr[1] + 1, ptr[2], ptr[2] + 100, ptr[2] + 256, ptr[3] + 2]] = True
    held = fix if fixed else np.zeros(N, dtype=bool)
    mask = rng.integers(0, 2, (B, 3, 3)).astype(np.float64)
    mask[0] = 0.0  # (with a pressure on, structure 0's cell rows feel no force)
    b = _block(rep, "alignn_fire_args").set(B=B, N=N, steps=2, nmin=5, fmax=0.05, maxstep=0.2, dtmax=1.0, finc=1.1, fdec=0.5, astart=0.1,
                                            fa=0.99, hydrostatic_strain=int(options), constant_volume=int(options))
    null = (() if cell else FILTER) + (() if options else OPTIONS) + (() if fixed else ("fixed",))
    steady = dict(atom_ptr=_t(ptr, I32), inv_lattice=_t(np.linalg.inv(lat0)), positions=_t(pos), velocities=torch.zeros(N, 3, dtype=F64, device=DEV),
                  state=_t([[0.1, 0.1]] * B), istate=torch.zeros(B, 2, dtype=I32, device=DEV))
    if cell:
        steady.update(lattice0=_t(lat0), xa=_t(pos), xc=torch.zeros(B, 3, 3, dtype=F64, device=DEV),
                      cell_velocities=torch.zeros(B, 3, 3, dtype=F64, device=DEV), defgrad=_t(np.stack([np.eye(3)] * B)), lattice=_t(lat0))
    if fixed:
        steady["fixed"] = _t(fix, U8)
    if options:
        steady.update(cell_mask=_t(mask), scalar_pressure=_t(rng.uniform(0.01, 0.05, B)))
    launches = [([2, 0, 3], [257, 1, 5], [2, 0, 1, 0]), ([2, 3], [257, 4], [1, 0, -1]), ([2, 3], [257, 5], [1, 2, 0])]
    plain, out_rows, out_structs, moved = {}, set(), set(), np.zeros(N, dtype=bool)
    for active, counts, status in launches:
        fp = _ptr(counts)
        forces = rng.normal(size=(int(fp[-1]), 3))
        stress = 0.01 * rng.normal(size=(len(active), 3, 3))
        for k, s in enumerate(active):
            if s == 0:
                forces[fp[k]:fp[k + 1]], stress[k] = 0.0, 0.0
        for f in PER_LAUNCH:
            b.payload.pop(f, None)
            plain.pop(f, None)
        b.set(n_active=len(active), force_rows=int(fp[-1]))
        inputs = dict(forces=_t(forces), energy=_t(rng.normal(size=len(active))), force_ptr=_t(fp, I32), active=_t(active, I32))
        if cell:
            inputs["stress"] = _t(stress)
        b.alloc("alignn_fire_step", dict(inputs, **steady), null)
        steady = {}
        plain.update({k: v for k, v in sx.plain_copy(b).items() if k not in plain})
        before = sx.plain_copy(b)
        _launch(b, lib, plain)
        assert b.payload["status"].tolist() == status, (b.payload["status"].tolist(), status)
        fits = [s for k, s in enumerate(active) if counts[k] == ns[s]]
        stepped = [s for s, f in zip(active, status[1:]) if f == 0]
        out_structs |= set(fits)
        moved |= _rows(ptr, stepped, skip=held).numpy()
        of = lambda w: _items(B, out_structs, w)  # noqa: E731
        on = lambda w: _items(B, stepped, w)  # noqa: E731
        written = dict(forces_out=_rows(ptr, out_structs, 3), energy_out=of(1), fmax_out=of(1), frac=torch.tensor(np.repeat(moved, 3)),
                       velocities=_rows(ptr, stepped, 3), state=on(2), istate=on(2),
                       positions=_rows(ptr, stepped, 3, skip=None if cell else held))
        if cell:
            written.update(stress_out=of(9), xa=_rows(ptr, stepped, 3, skip=held), xc=on(9), cell_velocities=on(9), defgrad=on(9), lattice=on(9))
        if options:
            written["enthalpy_out"] = of(1)
        _verify(b, plain, written, before)
    assert 1 not in out_structs and b.payload["istate"].view(-1, 2)[:, 1].tolist() == [0, 0, 2, 2]
    rep.finish()


# ======================================================================================================================
# MD
# ======================================================================================================================
MD_NS = [1, 2, 257]
FRAMES = ("epot", "ekin", "temperature", "pressure_out", "volume_out", "traj_positions", "traj_momenta", "traj_lattice", "conserved_out")
OPTIONAL = ("pressure_out", "volume_out", "traj_lattice", "noise_out", "conserved_out")
MD_CASES = [(e, o, f, 0.0) for e in range(6) for o, f in ((True, 1), (False, 0))] + [(6, True, 1, 40.0), (6, False, 0, 40.0), (6, True, 0, 0.0),
                                                                                    (6, False, 1, -1.0)]
# fixcm apart from the optional outputs, for the ensembles whose noise_out depends on it (Langevin's [N][18] does not, Andersen's
# last 12 of every 36 do) and for the chains, whose fixcm acts at t = 0 only
MD_CASES += [(1, True, 0, 0.0), (3, True, 0, 0.0), (1, False, 1, 0.0), (3, False, 1, 0.0), (5, True, 0, 0.0), (2, True, 0, 0.0)]


def _md_state(ens, ptime, t, steps):
    """per launch: which ``state`` arrays the header lets a launch of this ensemble rewrite"""
    begins, cell = t < steps, ens == 4 or (ens == 6 and ptime > 0.0)
    return dict(momenta=True, positions=begins, velocities=begins and ens in (1, 3), lattice=begins and cell, inv_lattice=begins and cell,
                nhc_state=ens in (5, 6))


def _md_frames(b, ens, fixcm, frames_written, begun):
    """cumulative: the elements of the ``out`` arrays that the launches so far have written"""
    has_cell = ens in (3, 4, 6)
    writes = dict(epot=True, ekin=True, temperature=True, traj_positions=True, traj_momenta=True, pressure_out=has_cell, volume_out=has_cell,
                  traj_lattice=has_cell, conserved_out=ens in (5, 6))
    out = {}
    for f in FRAMES:
        t = b.payload.get(f)
        if t is not None:
            m = torch.zeros(t.numel(), dtype=torch.bool)
            if writes[f]:
                m[:frames_written * (t.numel() // 3)] = True
            out[f] = m
    out["frac"] = begun
    if b.payload.get("noise_out") is not None:
        n = b.payload["noise_out"].numel()
        if ens == 1:
            out["noise_out"] = begun
        elif ens == 3:
            per = np.zeros(36, dtype=bool)
            per[:24 if not fixcm else 36] = begun
            out["noise_out"] = torch.tensor(np.tile(per, n // 36))
        else:
            out["noise_out"] = False
    return out


@pytest.mark.parametrize("ens,optional,fixcm,ptime", MD_CASES)
def test_md_step_between_guards(ens, optional, fixcm, ptime):
    """B = 3 of 1, 2 and 257 atoms, steps = 5, interval = 2: first one launch with n_rows = N + 1 (status -1, nothing else
    touched), then t = 0 .. 5 in order; the frames 0, 1, 2 are written by t = 0, 2, 4 and a launch with odd t leaves every frame
    array as it was."""
    lib, rng = _library(), np.random.default_rng(100 + ens)
    ns, ptr = MD_NS, _ptr(MD_NS)
    B, N, steps, interval = len(ns), int(ptr[-1]), 5, 2
    rep = _report(f"md ensemble={ens} optional={optional} fixcm={fixcm} ptime={ptime}")
    b = _block(rep, "alignn_md_args").set(n_structures=B, N=N, n_rows=N + 1, t=0, interval=interval, steps=steps, ensemble=ens, fixcm=fixcm,
                                          dt=0.5, friction=0.02, andersen_prob=0.3, taut=50.0, taup=100.0, kB=KB, chain=3, nhc_loops=2,
                                          nhc_order=3, ttime=25.0, ptime=ptime)
    lat = 8.0 * np.eye(3) + 0.3 * rng.normal(size=(B, 3, 3))
    needs_stress = optional or ens == 4 or (ens == 6 and ptime > 0.0)
    null = (() if optional else OPTIONAL) + (() if needs_stress else ("stress",))
    inputs = dict(forces=_t(0.1 * rng.normal(size=(N + 1, 3))), energy=_t(rng.normal(size=B)), stress=_t(0.01 * rng.normal(size=(B, 3, 3))),
                  atom_ptr=_t(ptr, I32), masses=_t(rng.uniform(1.0, 50.0, N)), t0_kelvin=_t(rng.uniform(200.0, 400.0, B)),
                  seeds=_t(rng.integers(1, 2 ** 62, B), I64), pressure=_t(rng.uniform(0.0, 1e-3, B)), compressibility=_t(rng.uniform(0.01, 0.05, B)),
                  lattice=_t(lat), inv_lattice=_t(np.linalg.inv(lat)), momenta=_t(rng.normal(size=(N, 3))), positions=_t(rng.uniform(0.0, 8.0, (N, 3))),
                  velocities=torch.zeros(N, 3, dtype=F64, device=DEV), nhc_state=torch.zeros(B, 34, dtype=F64, device=DEV))
    if not needs_stress:
        del inputs["stress"]
    b.alloc("alignn_md_step", inputs, null)
    plain = sx.plain_copy(b)
    # n_rows is not atom_ptr[B]: status[0] = -1 and every other array as it was
    before = sx.plain_copy(b)
    _launch(b, lib, plain)
    assert b.payload["status"].tolist() == [-1]
    nothing = {f: False for f, t in b.payload.items() if t is not None and b.role(f, "alignn_md_step") in ("out", "state")}
    _verify(b, plain, nothing, before)
    for p in (b.payload, plain):
        p["status"].zero_()
        p.pop("forces")
    b.set(n_rows=N).alloc("alignn_md_step", dict(forces=_t(np.zeros((N, 3)))), null)
    plain["forces"] = b.payload["forces"].clone()
    for t in range(steps + 1):
        f = _t(0.1 * rng.normal(size=(N, 3)))
        b.payload["forces"].copy_(f)
        plain["forces"].copy_(f)
        b.set(t=t)
        before = sx.plain_copy(b)
        _launch(b, lib, plain)
        assert b.payload["status"].tolist() == [0]
        written = dict(_md_state(ens, ptime, t, steps), **_md_frames(b, ens, fixcm, t // interval + 1, True))
        _verify(b, plain, written, before)
        if t % interval:
            for f in FRAMES:
                assert b.payload.get(f) is None or _eq(b.payload[f], before[f]), (t, f)
    rep.finish()


def test_md_init_momenta_between_guards():
    rng, ptr = np.random.default_rng(3), _ptr(MD_NS)
    rep = _report("md_init_momenta")
    _flat_case(rep, "alignn_md_init_momenta", dict(n_structures=3, kB=KB, N=int(ptr[-1])),
               dict(atom_ptr=_t(ptr, I32), masses=_t(rng.uniform(1.0, 50.0, int(ptr[-1]))), t_kelvin=_t([300.0, 10.0, 1000.0]),
                    seeds=_t(rng.integers(1, 2 ** 62, 3), I64)))
    rep.finish()


# ======================================================================================================================
# NEB and IDPP
# ======================================================================================================================
def _bands(shapes, seed, side=7.0):
    """random bands (n atoms, M images): cells, endpoints, interior rows and the index tables of alignn_neb.h"""
    rng = np.random.default_rng(seed)
    ns, Ms = [n for n, _ in shapes], [m for _, m in shapes]
    B = len(shapes)
    lat = side * np.eye(3) + 0.3 * rng.normal(size=(B, 3, 3))
    d = dict(ns=ns, Ms=Ms, B=B, lat=lat, inv=np.stack([_inv3_cof(c.reshape(-1)).reshape(3, 3) for c in lat]),
             end_ptr=_ptr(ns), row_ptr=_ptr([(m - 2) * n for n, m in shapes]), image_ptr=_ptr(Ms))
    d["initial"], d["final"] = rng.uniform(0.0, side, (sum(ns), 3)), rng.uniform(0.0, side, (sum(ns), 3))
    d["positions"] = rng.uniform(0.0, side, (int(d["row_ptr"][-1]), 3))
    return d, rng


def _evaluation(d, active, short=None):
    """force_ptr and energy_ptr of the active bands; band ``short`` gets one force row too few (it does not fit)"""
    rows = [(d["Ms"][s] - 2) * d["ns"][s] - (s == short) for s in active]
    return _ptr(rows), _ptr([d["Ms"][s] - 2 for s in active])


NEB_BANDS = [(1, 3), (5, 64), (257, 3)]  # 64: ALIGNN_NEB_MAX_IMAGES


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("climb", [0, 1])
@pytest.mark.parametrize("fixed", [False, True])
def test_neb_forces_between_guards(method, climb, fixed):
    """active = [2, 0]: the energies_out of the inactive band of 64 images keep the pattern; then active = [1, 0] with one force row
    too few for band 0: imax = -1 and the rest of it untouched, beside the band of 64 images"""
    lib = _library()
    d, rng = _bands(NEB_BANDS, 23)
    assert max(d["Ms"]) == _abi.header("alignn_neb.h").defines["ALIGNN_NEB_MAX_IMAGES"]
    N = int(d["row_ptr"][-1])
    fix = rng.integers(0, 4, N) == 0
    for active, short in (([2, 0], None), ([1, 0], 0)):
        rep = _report(f"neb method={method} climb={climb} fixed={fixed} active={active}")
        fp, ep = _evaluation(d, active, short)
        b = _block(rep, "alignn_neb_args").set(B=d["B"], N=N, n_ends=sum(d["ns"]), n_images=sum(d["Ms"]), n_active=len(active),
                                               force_rows=int(fp[-1]), n_energies=int(ep[-1]), max_images=max(d["Ms"][s] for s in active),
                                               method=method, climb=climb)
        inputs = dict(forces=_t(rng.normal(size=(int(fp[-1]), 3))), energy=_t(rng.normal(size=int(ep[-1]))), force_ptr=_t(fp, I32),
                      energy_ptr=_t(ep, I32), active=_t(active, I32), row_ptr=_t(d["row_ptr"], I32), image_ptr=_t(d["image_ptr"], I32),
                      end_ptr=_t(d["end_ptr"], I32), lattice=_t(d["lat"]), inv_lattice=_t(d["inv"]), spring=_t(rng.uniform(0.05, 0.5, d["B"])),
                      initial=_t(d["initial"]), final=_t(d["final"]), end_energy=_t(rng.normal(size=(d["B"], 2))), positions=_t(d["positions"]))
        if fixed:
            inputs["fixed"] = _t(fix, U8)
        b.alloc("alignn_neb_forces", inputs, () if fixed else ("fixed",))
        plain = sx.plain_copy(b)
        _launch(b, lib, plain)
        fits = [k for k, s in enumerate(active) if s != short]
        _verify(b, plain, dict(forces_out=_rows(fp, fits, 3), energies_out=_rows(d["image_ptr"], [active[k] for k in fits]),
                               emax=_items(len(active), fits)))
        imax = b.payload["imax"].tolist()
        assert all((imax[k] == -1) == (k not in fits) and (k not in fits or 1 <= imax[k] <= d["Ms"][s] - 2) for k, s in enumerate(active))
        rep.finish()


@pytest.mark.parametrize("with_inverse", [False, True])
def test_neb_interpolate_between_guards(with_inverse):
    d, _ = _bands(NEB_BANDS, 29)
    rep = _report(f"neb_interpolate inverse={with_inverse}")
    lat, initial, final = _t(d["lat"]), _t(d["initial"]), _t(d["final"])
    _, P = _flat_case(rep, "alignn_neb_interpolate", dict(n_bands=d["B"], n_rows=int(d["row_ptr"][-1]), n_ends=sum(d["ns"])),
                      dict(initial=initial, final=final, end_ptr=_t(d["end_ptr"], I32), lattice=lat, row_ptr=_t(d["row_ptr"], I32)),
                      () if with_inverse else ("inv_lattice",))
    out, inv = neb_interpolate(lat, initial, final, d["ns"], d["Ms"])  # the driver: one call is this launch
    assert _eq(P["positions"], out) and out.numel() == 3 * int(d["row_ptr"][-1])
    assert not with_inverse or (_eq(P["inv_lattice"], inv) and _eq(inv, _t(d["inv"])))
    rep.finish()


IDPP_BANDS = [(1, 3), (65, 4), (5, 64)]  # (1, 3): no pair at all; (65, 4): one b past a wavefront's stride


def test_idpp_forces_between_guards():
    """every band active (the driver's launch), an active subset out of order, and one band with a force row too few:
    status -1 and nothing of it written"""
    lib = _library()
    d, _ = _bands(IDPP_BANDS, 31)
    N = int(d["row_ptr"][-1])
    lat, initial, final, positions = _t(d["lat"]), _t(d["initial"]), _t(d["final"]), _t(d["positions"])
    energy, forces = idpp_forces(lat, initial, final, positions, d["ns"], d["Ms"])
    eptr = _ptr([m - 2 for m in d["Ms"]])
    for active, short in (([0, 1, 2], None), ([2, 0], None), ([1, 2, 0], 2)):
        rep = _report(f"idpp active={active} short={short}")
        fp, ep = _evaluation(d, active, short)
        b = _block(rep, "alignn_idpp_args").set(B=d["B"], N=N, n_ends=sum(d["ns"]), n_active=len(active), force_rows=int(fp[-1]),
                                                n_energies=int(ep[-1]), max_images=max(d["Ms"][s] for s in active),
                                                max_atoms=max(d["ns"][s] for s in active))
        b.alloc("alignn_idpp_forces", dict(force_ptr=_t(fp, I32), energy_ptr=_t(ep, I32), active=_t(active, I32), row_ptr=_t(d["row_ptr"], I32),
                                           end_ptr=_t(d["end_ptr"], I32), lattice=lat, inv_lattice=_t(d["inv"]), initial=initial, final=final,
                                           positions=positions))
        plain = sx.plain_copy(b)
        _launch(b, lib, plain)
        fits = [k for k, s in enumerate(active) if s != short]
        _verify(b, plain, dict(forces=_rows(fp, fits, 3), energy=_rows(ep, fits)))
        assert b.payload["status"].tolist() == [0 if k in fits else -1 for k in range(len(active))]
        for k in fits:  # the driver's bits: a band's results depend on its own rows alone
            s = active[k]
            assert _eq(b.payload["forces"][fp[k]:fp[k + 1]], forces[d["row_ptr"][s]:d["row_ptr"][s + 1]]), (active, s)
            assert _eq(b.payload["energy"][ep[k]:ep[k + 1]], energy[eptr[s]:eptr[s + 1]]), (active, s)
        if short is None and len(active) == d["B"]:
            assert forces.numel() == b.extent("forces")[0] and energy.numel() == b.extent("energy")[0]  # (d)
        rep.finish()


# ======================================================================================================================
# finite-displacement phonons
# ======================================================================================================================
def _phonon_batch():
    lib = _library()
    n_max = lib.alignn_phonon_eigh_max_dim() // 3
    ns, scs = [1, 3, n_max], [(2, 2, 2), (3, 1, 2), (1, 1, 1)]
    ncell = [int(np.prod(c)) for c in scs]
    ms = [3 * n for n in ns]
    return dict(ns=ns, scs=scs, ncell=ncell, ms=ms, ptr=_ptr(ns), fc_off=_ptr([c * m * m for c, m in zip(ncell, ms)]),
                n_sc=[n * c for n, c in zip(ns, ncell)])


@pytest.mark.parametrize("with_cart", [False, True])
@pytest.mark.parametrize("drift", [0, 1, 2])
def test_phonon_force_constant_launches_between_guards(with_cart, drift):
    """_displace, _fc_rows, _symmetrize, _acoustic and _mass_weight in the driver's order on structures of 1, 3 and the largest
    number of atoms the eigen launch takes, supercells (2, 2, 2), (3, 1, 2) and (1, 1, 1): max_elems and max_atoms come from the
    largest structure, so the small ones see a grid sized for another"""
    g, rng = _phonon_batch(), np.random.default_rng(41)
    ns, ptr, B, N = g["ns"], g["ptr"], 3, int(g["ptr"][-1])
    rep = _report(f"phonon fc cart={with_cart} drift={drift}")
    lat = 4.0 * np.eye(3) + 0.2 * rng.normal(size=(B, 3, 3))
    inv_super = np.stack([np.linalg.inv(np.diag(c) @ l) for c, l in zip(g["scs"], lat)])
    jobs = [(s, d) for s in range(B) for d in range(6 * ns[s])]
    row_off = _ptr([g["n_sc"][s] for s, _ in jobs])
    rows, fc_total = int(row_off[-1]), int(g["fc_off"][-1])
    common = dict(atom_ptr=_t(ptr, I32), supercell=_t(g["scs"], I32))
    pos, forces = rng.uniform(0.0, 4.0, (N, 3)), rng.normal(size=(rows, 3))
    _flat_case(rep, "alignn_phonon_displace", dict(n_jobs=len(jobs), delta=0.01, B=B, N=N, rows=rows),
               dict(common, positions=_t(pos), lattice=_t(lat), inv_supercell=_t(inv_super), jobs=_t(jobs, I32),
                    row_off=_t(row_off[:-1], I64)), () if with_cart else ("cart",), dict(frac=True, **({"cart": True} if with_cart else {})))
    pairs = [(s, x) for s in range(B) for x in range(3 * ns[s])]
    pair_rows = [row_off[jobs.index((s, 2 * x))] for s, x in pairs]
    fc_off = _t(g["fc_off"][:-1], I64)
    _, P = _flat_case(rep, "alignn_phonon_fc_rows", dict(n_pairs=len(pairs), drift=drift, delta=0.01, B=B, N=N, fc_total=fc_total, force_rows=rows),
                      dict(common, forces=_t(forces), pairs=_t(pairs, I32), pair_rows=_t(pair_rows, I64), fc_off=fc_off),
                      written=dict(fc=True))
    sizes = dict(n_structures=B, B=B, N=N, fc_total=fc_total)
    max_elems = max(c * m * m for c, m in zip(g["ncell"], g["ms"]))
    _, P = _flat_case(rep, "alignn_phonon_symmetrize", dict(sizes, max_elems=max_elems), dict(common, fc_in=P["fc"], fc_off=fc_off))
    diagonal = torch.zeros(fc_total, dtype=torch.bool)
    for s in range(B):
        m = g["ms"][s]
        for a in range(ns[s]):
            for i in range(3):
                at = int(g["fc_off"][s]) + (3 * a + i) * m + 3 * a
                diagonal[at:at + 3] = True
    lib = _library()
    c = _call(rep, "alignn_phonon_acoustic").set(max_atoms=max(ns), **sizes).alloc(dict(common, fc=P["fc_out"], fc_off=fc_off))
    plain = sx.plain_copy(c)
    before = sx.plain_copy(c)
    _launch(c, lib, plain)
    _verify(c, plain, dict(fc=diagonal), before)
    masses = rng.uniform(1.0, 200.0, N)
    _, D = _flat_case(rep, "alignn_phonon_mass_weight", dict(sizes, max_elems=max_elems),
                      dict(common, fc=c.payload["fc"], masses=_t(masses), fc_off=fc_off))
    if with_cart and drift == 1:  # the driver on a forces_fn: this sequence in one chunk, then _eigh with its scale
        q = rng.uniform(-0.5, 0.5, (3, 3))
        ms, R = g["ms"], np.concatenate([lattice_points(s) for s in g["scs"]])
        freq_off, mode_off = 3 * _ptr(ms), 6 * _ptr([m * m for m in ms])
        _, E = _flat_case(rep, "alignn_phonon_eigh",
                          dict(n_structures=B, max_dim=max(ms), n_q=3, scale=FREQ_SCALE, dyn_total=fc_total, n_points=len(R), sum_m=sum(ms),
                               sum_mm=sum(m * m for m in ms)),
                          dict(dyn=D["dyn"], dyn_off=fc_off, lattice_points=_t(R, I32), cell_ptr=_t(_ptr(g["ncell"]), I32), dims=_t(ms, I32),
                               qpoints=_t(q), freq_off=_t(freq_off[:-1], I64), mode_off=_t(mode_off[:-1], I64)), ("eigvals",))
        split = lambda x: [x[ptr[s]:ptr[s + 1]] for s in range(B)]  # noqa: E731
        res = phonons(None, list(lat), split(pos), None, split(masses), supercell=g["scs"], delta=0.01, drift="frederiksen", symmetrize=1,
                      acoustic=True, qpoints=q, modes=True, dos_kpts=None, device=DEV,
                      forces_fn=lambda lats, carts: (torch.zeros(len(lats), dtype=F64, device=DEV), _t(forces)))
        assert res.n_evals == 1 and res.n_supercells == len(jobs)
        for s in range(B):
            assert _eq(c.payload["fc"][g["fc_off"][s]:g["fc_off"][s + 1]], res.force_constants[s]), s
            assert _eq(E["freqs"][freq_off[s]:freq_off[s + 1]], res.frequencies[s]), s
            assert _eq(E["modes"].reshape(-1)[mode_off[s]:mode_off[s + 1]], torch.view_as_real(res.modes[s].contiguous())), s
        assert sum(f.numel() for f in res.force_constants) == c.extent("fc")[0]  # (d)
    rep.finish()


@pytest.mark.parametrize("n_q", [1, 3])
@pytest.mark.parametrize("with_eigvals", [False, True])
@pytest.mark.parametrize("with_modes", [False, True])
def test_phonon_eigh_and_dos_between_guards(n_q, with_eigvals, with_modes):
    """dimensions 3, 9 and the maximum in one launch, and a fourth structure of dimension 3 with the 210 lattice points of a
    (5, 6, 7) supercell - more than one staged chunk; then _dos with 64 points on the frequencies"""
    g, rng = _phonon_batch(), np.random.default_rng(43)
    ms, ncell = g["ms"] + [3], g["ncell"] + [210]
    B = len(ms)
    rep = _report(f"phonon eigh n_q={n_q} eigvals={with_eigvals} modes={with_modes}")
    dyn_off = _ptr([c * m * m for c, m in zip(ncell, ms)])
    R = np.concatenate([lattice_points(c) for c in g["scs"] + [(5, 6, 7)]])
    assert len(R) == sum(ncell)
    freq_off, mode_off = n_q * _ptr(ms), 2 * n_q * _ptr([m * m for m in ms])
    null = (() if with_eigvals else ("eigvals",)) + (() if with_modes else ("modes",))
    c, P = _flat_case(rep, "alignn_phonon_eigh",
                      dict(n_structures=B, max_dim=max(ms), n_q=n_q, scale=1.0, dyn_total=int(dyn_off[-1]), n_points=len(R), sum_m=sum(ms),
                           sum_mm=sum(m * m for m in ms)),
                      dict(dyn=_t(rng.normal(size=int(dyn_off[-1]))), dyn_off=_t(dyn_off[:-1], I64), lattice_points=_t(R, I32),
                           cell_ptr=_t(_ptr(ncell), I32), dims=_t(ms, I32), qpoints=_t(rng.uniform(-0.5, 0.5, (n_q, 3))),
                           freq_off=_t(freq_off[:-1], I64), mode_off=_t(mode_off[:-1], I64)), null)
    assert P["status"].tolist() == [0] and bool(torch.isfinite(P["freqs"]).all())
    for s in range(B):  # ascending per q
        f = P["freqs"][freq_off[s]:freq_off[s + 1]].view(n_q, ms[s])
        assert bool((f[:, 1:] >= f[:, :-1]).all()), s
    _flat_case(rep, "alignn_phonon_dos", dict(n_structures=B, npts=64, width=0.05, n_freqs=int(freq_off[-1])),
               dict(freqs=P["freqs"], freq_off=_t(freq_off, I64)))
    rep.finish()


# ======================================================================================================================
# builders
# ======================================================================================================================
def _parents():
    ps = [defects_ref.fcc(4.0), interface_ref.triclinic()]
    ptr = _ptr([len(p) for _, p in ps])
    return ps, ptr, dict(positions=_t(np.concatenate([p for _, p in ps])), atom_ptr=_t(ptr, I32), lattice=_t(np.stack([l for l, _ in ps])))


def test_defect_supercells_between_guards():
    """a = -1 and a >= 0 jobs of two parents, and one job whose row range is one row short: nothing of it is written"""
    ps, ptr, parents = _parents()
    dims = [(2, 1, 2), (1, 2, 1)]
    n_sc = [len(p) * int(np.prod(d)) for (_, p), d in zip(ps, dims)]
    jobs = [(0, -1), (0, 5), (1, -1), (1, 3), (0, 2), (1, n_sc[1] - 1)]
    counts = [n_sc[s] - (a >= 0) for s, a in jobs]
    counts[4] -= 1  # does not fit
    fits, off = [0, 1, 2, 3, 5], _ptr(counts)
    rep = _report("defect_supercells")
    _, P = _flat_case(rep, "alignn_defect_supercells", dict(n_structures=2, n_jobs=len(jobs), N=int(ptr[-1]), rows=int(off[-1])),
                      dict(parents, supercell=_t(dims, I32), jobs=_t(jobs, I32), row_off=_t(off, I64)),
                      written=dict(cells=_items(len(jobs), fits, 9), cart=_rows(off, fits, 3), frac=_rows(off, fits, 3), src=_rows(off, fits)))
    for k in fits:  # the restatement, which tests/test_gpu_defects.py ties the kernel to
        s, a = jobs[k]
        want = defects_ref.supercell(ps[s][0], ps[s][1], dims[s], a, beg=ptr[s])
        assert np.array_equal(P["cart"][off[k]:off[k + 1]].cpu().numpy(), want[1]) and np.array_equal(P["cells"].view(-1, 3, 3)[k].cpu().numpy(), want[0])
    rep.finish()


def test_slab_and_strain_builders_between_guards():
    ps, ptr, parents = _parents()
    rng = np.random.default_rng(47)
    rep = _report("slab_build, strain_build")
    jobs, counts = [], []
    for s, (l, p) in enumerate(ps):
        for hkl, layers in (((1, 0, 0), 1), ((1, 1, 1), 3)):
            jobs.append([s] + [int(v) for v in defects_ref.miller_basis(l, hkl).reshape(-1)] + [layers])
            counts.append(len(p) * layers)
    jobs.append(list(jobs[1]))
    counts.append(counts[1] + 1)  # does not fit
    off, fits = _ptr(counts), [0, 1, 2, 3]
    _, S = _flat_case(rep, "alignn_slab_build", dict(n_structures=2, n_jobs=len(jobs), N=int(ptr[-1]), rows=int(off[-1])),
                      dict(parents, jobs=_t(jobs, I32), vacuum=_t(np.full(len(jobs), 7.5)), row_off=_t(off, I64)),
                      written=dict(cells=_items(len(jobs), fits, 9), cart=_rows(off, fits, 3), frac=_rows(off, fits, 3), src=_rows(off, fits)))
    packed = pack([l for l, _ in ps], [p for _, p in ps], [len(p) for _, p in ps], torch.device(DEV), frac=False)
    cells, cart, src, off_d = build_slabs(packed, jobs[:4], counts[:4], 7.5, torch.device(DEV))  # the driver: one call is this launch
    end = int(off[4])
    assert off_d.tolist() == off[:5].tolist() and cart.numel() == 3 * end  # (d), over the jobs that fit
    assert _eq(S["cells"][:12], cells) and _eq(S["cart"][:end], cart) and _eq(S["src"][:end], src)
    # alignn_strain_build: both parents under two deformations, in the driver's order, and one job with two rows too many
    F = np.eye(3) + 0.03 * rng.normal(size=(2, 3, 3))
    sjobs = [0, 0, 1, 1, 0]
    counts = [len(ps[s][1]) for s in sjobs]
    counts[4] += 2  # does not fit
    off, fits = _ptr(counts), [0, 1, 2, 3]
    _, S = _flat_case(rep, "alignn_strain_build", dict(n_structures=2, n_jobs=len(sjobs), N=int(ptr[-1]), rows=int(off[-1])),
                      dict(parents, jobs=_t(sjobs, I32), defgrad=_t(np.concatenate([F, F, F[:1]])), row_off=_t(off, I64)),
                      written=dict(cells=_items(len(sjobs), fits, 9), cart=_rows(off, fits, 3), volume=_items(len(sjobs), fits)))
    cells, cart, volumes, _, n = strain_jobs(packed, [len(p) for _, p in ps], _t(F), torch.device(DEV))  # the driver: this launch
    end = int(off[4])
    assert n == counts[:4] and cart.numel() == 3 * end  # (d)
    assert _eq(S["cells"][:12], cells) and _eq(S["cart"][:end], cart) and _eq(S["volume"][:4], volumes)
    rep.finish()


def _guarded_match(rep, films, subs, kw):
    """``alignn_zsl_match`` between guards, every workspace at its stated extent -> (the call, its payload, the restated statuses)"""
    want = [interface_ref.match(f, s, **kw)["status"] for f, s in zip(films, subs)]
    P = len(films)
    hnf, prefix = interface_ref.hnf_tables()
    nmax = np.zeros((P, 2), dtype=np.int32)
    for p in range(P):
        if interface_ref.cell_valid(films[p]) and interface_ref.cell_valid(subs[p]):
            nmax[p] = [interface_ref.largest_multiple(interface_ref.cross2(c), kw["max_area"]) for c in (films[p], subs[p])]
    off = np.concatenate([[[0, 0]], np.cumsum(prefix[nmax + 1].astype(np.int64), axis=0)])
    ok = [p for p in range(P) if want[p] == 0]
    c, out = _flat_case(rep, "alignn_zsl_match",
                        dict(n_pairs=P, max_film=int(nmax[:, 0].max()), max_subs=int(nmax[:, 1].max()), film_rows=int(off[-1, 0]),
                             subs_rows=int(off[-1, 1]), max_area_ratio_tol=kw["max_area_ratio_tol"], ltol=kw["ltol"],
                             cos_atol=interface_ref.cos_of_degrees(kw["atol"]), n_hnf=len(hnf)),
                        dict(film_cells=_t(np.stack(films)), subs_cells=_t(np.stack(subs)), nmax_film=_t(nmax[:, 0], I32),
                             nmax_subs=_t(nmax[:, 1], I32), hnf=_t(hnf, I32), prefix=_t(prefix, I32), film_off=_t(off[:-1, 0], I64),
                             subs_off=_t(off[:-1, 1], I64)),
                        written=dict(multiples=_items(P, ok, 2), film_matrix=_items(P, ok, 4), subs_matrix=_items(P, ok, 4),
                                     mismatch=_items(P, ok, 4)))
    assert out["status"].tolist() == want and len(prefix) == c.extent("prefix")[0] and int(prefix[-1]) == len(hnf)
    res = match_lattices(np.stack(films), np.stack(subs), device=DEV, **kw)  # the driver: one chunk, this launch
    assert res.status.tolist() == want
    for p in ok:
        assert out["multiples"].view(-1, 2)[p].tolist() == [res.film_multiple[p], res.subs_multiple[p]]
        assert np.array_equal(out["film_matrix"].view(-1, 2, 2)[p].cpu().numpy(), res.film_matrix[p])
        assert np.array_equal(out["subs_matrix"].view(-1, 2, 2)[p].cpu().numpy(), res.subs_matrix[p])
        assert out["mismatch"].view(-1, 4)[p, 3].item() == res.score[p]
    return c, out, want


def test_zsl_match_between_guards():
    """statuses 0, 1 and 2 in one launch, every workspace at its stated extent; nothing but the status of a pair with status != 0"""
    kw = dict(max_area=30.0, max_area_ratio_tol=1.0, ltol=0.01, atol=0.2)
    cell, mirror = np.array([[3.0, 0.0], [0.9, 2.6]]), np.array([[3.0, 0.0], [-0.9, 2.6]])
    bad = np.array([[3.0, np.nan], [0.0, 3.0]])
    films = [cell, cell, bad, interface_ref.hexagonal(2.9), cell @ interface_ref.rot(0.4)]
    subs = [cell, mirror, cell, 3.6 * np.eye(2), cell]
    rep = _report("zsl_match")
    _, _, want = _guarded_match(rep, films, subs, kw)
    assert set(want) == {0, 1, 2}
    rep.finish()


def _guarded_interfaces(rep, slabs, jobs, counts):
    """``alignn_interface_build`` between guards on ``jobs`` and, last, the first of them once more with row ranges that disagree
    (nothing of it is written); the pairs that fit are held to the restatement, which tests/test_gpu_interface.py ties the kernel to"""
    jobs, counts = jobs + [list(jobs[0])], counts + [counts[0], counts[1] + 1, counts[2] + 1]
    K, off, slab_off = len(jobs), _ptr(counts), _ptr([len(s[1]) for s in slabs])
    fits = list(range(K - 1))
    triples = [3 * k + q for k in fits for q in range(3)]
    rng = np.random.default_rng(53)
    sep, vac = rng.uniform(1.5, 3.0, K), rng.uniform(6.0, 9.0, K)
    _, P = _flat_case(rep, "alignn_interface_build", dict(n_slabs=len(slabs), n_pairs=K, slab_rows=int(slab_off[-1]), rows=int(off[-1])),
                      dict(slab_cells=_t(np.stack([s[0] for s in slabs])), slab_cart=_t(np.concatenate([s[1] for s in slabs])),
                           slab_off=_t(slab_off, I64), slab_src=_t(np.concatenate([s[2] for s in slabs]), I32), jobs=_t(jobs, I32),
                           separation=_t(sep), vacuum=_t(vac), out_off=_t(off, I64)),
                      written=dict(cells=_items(3 * K, triples, 9), cart=_rows(off, triples, 3), frac=_rows(off, triples, 3),
                                   src=_rows(off, triples), part=_rows(off, triples), area=_items(K, fits)))
    for k in fits:
        job = jobs[k]
        want = interface_ref.interface(slabs[job[0]], slabs[job[1]], job[2:6], job[6:10], sep[k], vac[k])
        assert P["area"][k].item() == want[5] and np.array_equal(P["cart"][off[3 * k + 2]:off[3 * k + 3]].cpu().numpy(), want[1][2])
        assert np.array_equal(P["cells"].view(-1, 3, 3)[3 * k].cpu().numpy(), want[0])


def _slabs(keys):
    parents = {"fcc": (defects_ref.fcc(4.0), 0), "tri": (interface_ref.triclinic(), 4)}
    return [interface_ref.ref_slab(parents[p][0], hkl, layers, parents[p][1]) for p, hkl, layers in keys]


def test_interface_build_between_guards():
    """the builder cases of tests/interface_ref.py (matrices with b != 0, reduced ones, variants that swap the vectors), and one
    pair that does not fit"""
    keys, jobs, counts = [], [], []
    for fp, fh, fl, sp, sh, sl, Mf, Ms in interface_ref.BUILDER_CASES:
        for key in ((fp, fh, fl), (sp, sh, sl)):
            if key not in keys:
                keys.append(key)
    slabs = _slabs(keys)
    for fp, fh, fl, sp, sh, sl, Mf, Ms in interface_ref.BUILDER_CASES:
        f, s = keys.index((fp, fh, fl)), keys.index((sp, sh, sl))
        jobs.append([f, s] + list(np.array(Mf).reshape(-1)) + list(np.array(Ms).reshape(-1)))
        n_s, n_f = round(np.linalg.det(Ms)) * len(slabs[s][1]), round(np.linalg.det(Mf)) * len(slabs[f][1])
        counts += [n_s, n_f, n_s + n_f]
    rep = _report("interface_build")
    _guarded_interfaces(rep, slabs, jobs, counts)
    rep.finish()


def test_matched_pairs_go_from_the_matcher_to_the_interface_builder_between_guards():
    """the driver's chain: the plane cells of vacuum-free slabs to ``alignn_zsl_match``, the matrices and multiples it wrote for
    the pairs of status 0 - read from the guarded buffers - as the jobs of ``alignn_interface_build``, plus one pair that does not
    fit"""
    slabs = _slabs([("fcc", (1, 0, 0), 1), ("fcc", (1, 0, 0), 3), ("fcc", (1, 1, 1), 3), ("tri", (1, 0, 0), 1), ("fcc", (1, 1, 0), 3)])
    planes = [_plane_cell(s[0]) for s in slabs]
    pairs = [(0, 1), (2, 3), (4, 1), (3, 4), (2, 1)]
    kw = dict(max_area=120.0, max_area_ratio_tol=0.1, ltol=0.08, atol=4.0)
    rep = _report("zsl_match, then interface_build")
    _, out, want = _guarded_match(rep, [planes[f] for f, _ in pairs], [planes[s] for _, s in pairs], kw)
    assert want.count(0) >= 4
    mult, fm, sm = (out[k].cpu().numpy() for k in ("multiples", "film_matrix", "subs_matrix"))
    jobs, counts = [], []
    for p, (f, s) in enumerate(pairs):
        if want[p] == 0:
            i, j = (int(v) for v in mult.reshape(-1, 2)[p])
            jobs.append([f, s] + [int(v) for v in fm.reshape(-1, 4)[p]] + [int(v) for v in sm.reshape(-1, 4)[p]])
            counts += [j * len(slabs[s][1]), i * len(slabs[f][1]), j * len(slabs[s][1]) + i * len(slabs[f][1])]
    assert any(job[2:6] != [1, 0, 0, 1] for job in jobs)  # (not only the trivial match)
    _guarded_interfaces(rep, slabs, jobs, counts)
    rep.finish()


# ======================================================================================================================
# fits
# ======================================================================================================================
def _padded(sets, ld, width):
    out = np.full((len(sets), ld) + width, -7.0)
    for s, x in enumerate(sets):
        out[s, :len(x)] = x
    return out


@pytest.mark.parametrize("form", sorted(EOS_FORMS))
@pytest.mark.parametrize("ld,ragged", [(4, False), (64, True), (64, False)])
def test_eos_fit_between_guards(form, ld, ragged):
    f = eos_ref.FORMS[form]
    sets = dict(eos_ref.synthetic_sets(f))
    if ld == 4:
        data = [sets["k4"], sets["k4_noise"], eos_ref.concave(eos_ref.DX_4)]
    elif ragged:  # one structure below 4 points: status 2
        data = list(sets.values()) + [eos_ref.concave(), (sets["k5"][0][:3], sets["k5"][1][:3])]
    else:
        V = 64.0 * (1.0 + np.linspace(-0.05, 0.05, 64)) ** 3
        E = eos_ref.ASE_FORMS[f](V, *eos_ref.TRUE)
        data = [(V, E), (V, E + np.random.default_rng(5).normal(0.0, 1e-4, 64)), (V, -V * V)]
    B = len(data)
    vol, en = _t(_padded([V for V, _ in data], ld, ())), _t(_padded([E for _, E in data], ld, ()))
    n = _t([len(V) for V, _ in data], I32) if ragged else None
    rep = _report(f"eos_fit {form} ld={ld} ragged={ragged}")
    inputs = dict(volume=vol, energy=en)
    if ragged:
        inputs["n_points"] = n
    _, P = _flat_case(rep, "alignn_eos_fit", dict(n_structures=B, ld=ld, form=EOS_FORMS[form]), inputs, () if ragged else ("n_points",))
    for got, want in zip((P["params"], P["rms"], P["n_iter"], P["status"]), eos_fit(vol, en, form, n)):  # the driver: this launch
        assert _eq(got, want)
    status = P["status"].tolist()
    assert 0 in status and 2 in status and (not ragged or status[-1] == 2)
    rep.finish()


@pytest.mark.parametrize("ld,ragged", [(7, False), (64, True), (64, False)])
def test_elastic_fit_between_guards(ld, ragged):
    sets = dict(elastic_ref.synthetic_sets())
    if ld == 7:
        data = [sets["p7"], sets["p7_noise"]]
    elif ragged:  # one crystal below 7 points: status 2
        data = list(sets.values()) + [elastic_ref.unstable_set(), elastic_ref.deficient_set(), (sets["p7"][0][:6], sets["p7"][1][:6])]
    else:
        C, sigma0 = elastic_ref.planted()
        e = 0.01 * np.random.default_rng(7).uniform(-1.0, 1.0, (64, 6))
        data = [(e, elastic_ref._stresses(C, sigma0, e)), (e[::-1].copy(), elastic_ref._stresses(C, sigma0, e[::-1]))]
    B = len(data)
    strain, stress = _t(_padded([e for e, _ in data], ld, (6,))), _t(_padded([g for _, g in data], ld, (3, 3)))
    n = _t([len(e) for e, _ in data], I32) if ragged else None
    rep = _report(f"elastic_fit ld={ld} ragged={ragged}")
    inputs = dict(strain=strain, stress=stress)
    if ragged:
        inputs["n_points"] = n
    _, P = _flat_case(rep, "alignn_elastic_fit", dict(n_structures=B, ld=ld), inputs, () if ragged else ("n_points",))
    names = ("c_raw", "c", "compliance", "sigma0", "moduli", "rms", "asymmetry", "status")
    for name, want in zip(names, elastic_fit(strain, stress, n)):  # the driver: this launch
        assert _eq(P[name], want), name
    assert not ragged or P["status"].tolist()[-3:] == [1, 2, 2]
    rep.finish()


# ======================================================================================================================
# thermodynamics
# ======================================================================================================================
TEMPERATURES, CUTOFF = np.array([0.0, 1e-3, 10.0, 300.0, 1e6]), 0.004


def _mesh_sets():
    """the sets of tests/test_gpu_thermo.py: (frequencies [Nq, m], Nq) with (m, Nq) = (3, 1), (9, 7), (96, 64) - six whole chunks
    of 1024 - and (25, 41): one chunk plus one mode; each with imaginary modes, exact zeros and modes exactly at the cutoff"""
    rng = np.random.default_rng(11)
    out = []
    for m, nq in ((3, 1), (9, 7), (96, 64), (25, 41)):
        f = rng.uniform(-0.01, 0.08, (nq, m))
        flat = f.reshape(-1)
        idx = rng.permutation(flat.size)[:max(4, flat.size // 20)]
        flat[idx[::2]], flat[idx[1::2]] = 0.0, CUTOFF
        out.append((f, nq))
    out[0] = (np.array([[-0.003, CUTOFF, 0.031]]), 1)
    assert [f.size for f, _ in out] == [3, 63, 6144, 1025]
    return out


def _derive_inputs(P, NT, seed):
    """the inputs of tests/test_gpu_thermo.py: B = 3 structures of P volume points and NT temperatures, smooth Cv(V) and S(V)
    with noise, one fitted volume outside the range, a fit with status 1 and, for NT = 3, one with status 2 (NaN parameters)"""
    rng = np.random.default_rng(seed)
    B = 3
    T = np.array([300.0, 450.0, 700.0])[:NT]
    V = np.stack([rng.uniform(40.0, 90.0) * (1.0 + np.linspace(-0.05, 0.06, P)) ** 3 for _ in range(B)])
    u = (V - V.mean(1, keepdims=True)) / np.ptp(V, axis=1, keepdims=True)
    cv = 2e-4 * (1.0 + 0.3 * u + 0.1 * u * u)[:, :, None] * (1.0 + 0.1 * np.arange(NT)) + rng.normal(0, 1e-7, (B, P, NT))
    s = 5e-4 * (1.0 + 0.5 * u - 0.2 * u * u)[:, :, None] * (1.0 + 0.3 * np.arange(NT)) + rng.normal(0, 1e-7, (B, P, NT))
    v_eq = V.mean(1, keepdims=True) * (1.0 + 0.004 * np.arange(NT)[None, :] + rng.uniform(-0.001, 0.001, (B, NT)))
    v_eq[2, -1] = V[2].max() * 1.01
    b_t = rng.uniform(0.3, 0.8, (B, NT))
    status = np.zeros((B, NT), dtype=np.int32)
    status[0, 0] = 1
    if NT == 3:
        status[1, 1] = 2
        v_eq[1, 1] = b_t[1, 1] = np.nan
    return V, cv, s, T, v_eq, b_t, status


@pytest.mark.parametrize("n_temps", [1, 5])
def test_phonon_thermal_between_guards(n_temps):
    """3, 63, 6144 and 1025 frequencies in one launch; the workspace guarded at exactly the byte count the library returns"""
    lib = _library()
    sets = _mesh_sets()
    T = TEMPERATURES if n_temps == 5 else np.array([300.0])
    off = _ptr([f.size for f, _ in sets])
    flat, nq = _t(np.concatenate([f.reshape(-1) for f, _ in sets])), np.array([q for _, q in sets])
    B, max_freqs = len(sets), int(np.diff(off).max())
    n_bytes = lib.alignn_phonon_thermal_workspace(B, max_freqs, n_temps)
    rep = _report(f"phonon_thermal n_temps={n_temps}")
    c, P = _flat_case(rep, "alignn_phonon_thermal",
                      dict(n_structures=B, max_freqs=max_freqs, n_temps=n_temps, cutoff=CUTOFF, workspace_bytes=n_bytes, n_freqs=int(off[-1])),
                      dict(freqs=flat, freq_off=_t(off, I64), n_q=_t(nq, I32), temperatures=_t(T)))
    assert P["workspace"].numel() == n_bytes > 0
    names = ("free_energy", "internal_energy", "entropy", "heat_capacity", "zpe", "n_skipped")
    for name, want in zip(names, thermal_sums(flat, off, nq, T, CUTOFF)):  # the driver: this launch
        assert _eq(P[name], want), name
    rep.finish()


@pytest.mark.parametrize("P", [4, 64])
@pytest.mark.parametrize("NT", [1, 3])
def test_qha_derive_between_guards(P, NT):
    V, cv, s, T, v_eq, b_t, status = _derive_inputs(P, NT, 100 * P + NT)
    ins = dict(volumes=_t(V), heat_capacity=_t(cv), entropy=_t(s), temperatures=_t(T), v_eq=_t(v_eq), b_t=_t(b_t), status=_t(status, I32))
    rep = _report(f"qha_derive P={P} NT={NT}")
    _, out = _flat_case(rep, "alignn_qha_derive", dict(n_structures=len(V), n_points=P, n_temps=NT), ins)
    names = ("alpha", "cv_out", "s_out", "cp_out", "gamma", "inside")
    for name, want in zip(names, qha_derive(*ins.values())):  # the driver: this launch
        assert _eq(out[name], want), name
    rep.finish()


# ======================================================================================================================
# the flat entry points of alignn_traj.h
# ======================================================================================================================
@pytest.mark.parametrize("n_rows", [1, 7])
@pytest.mark.parametrize("n_freq", [1, 256])
def test_flat_trajectory_launches_between_guards(n_rows, n_freq):
    """a short max_lag; one row of the velocity autocorrelation starts at zero (zeros out); n_freq = 1 is below the header's
    n_freq >= 2: hipErrorInvalidValue, and nothing is written"""
    K, dtau = 3, 2.0
    rng = np.random.default_rng(59)
    vacf = rng.normal(size=(n_rows, K + 1))
    vacf[-1, 0] = 0.0 if n_rows > 1 else 1.5
    rep = _report(f"traj flat n_rows={n_rows} n_freq={n_freq}")
    sizes = dict(n_rows=n_rows, max_lag=K, dtau=dtau)
    valid = n_freq >= 2
    _, P = _flat_case(rep, "alignn_traj_vdos", dict(sizes, n_freq=n_freq, f_max_thz=30.0, window=1), dict(vacf=_t(vacf)),
                      written=dict(out=valid), expect=0 if valid else 1)
    if valid:
        assert _eq(P["out"], vdos(_t(vacf).view(1, n_rows, K + 1), dtau, n_freq=n_freq, f_max_THz=30.0, window="hann").dos)  # the driver
        assert n_rows == 1 or not bool(P["out"][-1].any())
    _flat_case(rep, "alignn_traj_fit", dict(sizes, k_lo=1, k_hi=K), dict(msd=_t(rng.uniform(0.0, 2.0, (n_rows, K + 1, 3)))))
    _, P = _flat_case(rep, "alignn_traj_green_kubo", dict(sizes, time_unit=FS), dict(vacf=_t(vacf)))
    assert _eq(P["out"], green_kubo(_t(vacf).view(1, n_rows, K + 1), dtau))  # the driver
    rep.finish()
