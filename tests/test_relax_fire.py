"""Checks of ``FireRef`` and ``run_ref`` of tests/relax_ref.py, the float64 numpy restatement of ASE's FIRE and ``Optimizer.run``
that specifies ``alignn_amd.relax`` (csrc/relax.hip): steps computed by hand on a 1-D harmonic well, and what the entry point
refuses before it touches a device.  The GPU tests (test_gpu_relax.py) hold the kernel and the batched relaxer to the
restatement."""

import numpy as np
import pytest

from alignn_amd.relax import RelaxResult, relax  # the batched relaxer the restatement specifies
from tests.relax_ref import FireRef, run_ref, well


def test_first_step_has_no_mixing():
    opt = FireRef([[1.0, 0.0, 0.0]])
    opt.step(well(1.0)(opt.r)[1])  # f = -1: v = 0 + 0.1 * -1, dr = 0.1 * v
    assert opt.v[0, 0] == pytest.approx(-0.1, abs=1e-15) and opt.r[0, 0] == pytest.approx(0.99, abs=1e-15)
    assert (opt.dt, opt.a, opt.Nsteps) == (0.1, 0.1, 0)


def test_second_step_mixes():
    opt = FireRef([[1.0, 0.0, 0.0]])
    ef = well(1.0)
    opt.step(ef(opt.r)[1])
    opt.step(ef(opt.r)[1])
    # f = -0.99, v = -0.1, P = 0.099 > 0: v = 0.9 (-0.1) + 0.1 (-0.99 / 0.99) 0.1 = -0.1; Nsteps 1 (not > Nmin: dt kept);
    # v += 0.1 (-0.99) -> -0.199; x = 0.99 - 0.0199
    assert opt.Nsteps == 1 and opt.dt == 0.1 and opt.a == 0.1
    assert opt.v[0, 0] == pytest.approx(-0.199, abs=1e-15) and opt.r[0, 0] == pytest.approx(0.9701, abs=1e-15)
    # across directions the mix turns v toward F, keeping |v|: v = [1, 0, 0], f = [1, 1, 0]
    o2 = FireRef([[0.0, 0.0, 0.0]])
    o2.v = np.array([[1.0, 0.0, 0.0]])
    o2.step(np.array([[1.0, 1.0, 0.0]]))
    c = 0.1 / np.sqrt(2.0)
    assert o2.v[0] == pytest.approx([0.9 + c + 0.1, c + 0.1, 0.0], abs=1e-15)


def test_dt_grows_after_nmin_downhill_steps():
    opt = FireRef([[1.0, 0.0, 0.0]])
    ef = well(1.0)
    for k in range(1, 8):  # step 1 starts the velocity, steps 2..7 are downhill with Nsteps 0..5 (not > Nmin = 5)
        opt.step(ef(opt.r)[1])
        assert opt.dt == 0.1 and opt.a == 0.1 and opt.Nsteps == k - 1
    opt.step(ef(opt.r)[1])  # step 8: Nsteps 6 > 5
    assert opt.dt == pytest.approx(0.11, abs=1e-15) and opt.a == pytest.approx(0.099, abs=1e-15) and opt.Nsteps == 7
    for _ in range(40):
        opt.step(ef(opt.r)[1])
        assert opt.dt <= 1.0  # dtmax


def test_maxstep_clip_then_uphill_reset():
    opt = FireRef([[0.1, 0.0, 0.0]])
    ef = well(300.0)
    opt.step(ef(opt.r)[1])  # f = -30, v = -3, dr = -0.3 -> clipped to -0.2
    assert opt.v[0, 0] == pytest.approx(-3.0, abs=1e-14) and opt.r[0, 0] == pytest.approx(-0.1, abs=1e-15)
    opt.step(ef(opt.r)[1])  # f = +30 against v = -3: P < 0 -> v = 0, a = astart, dt = 0.05, Nsteps = 0; v = 1.5, dr = 0.075
    assert (opt.a, opt.Nsteps) == (0.1, 0) and opt.dt == pytest.approx(0.05, abs=1e-16)
    assert opt.v[0, 0] == pytest.approx(1.5, abs=1e-14) and opt.r[0, 0] == pytest.approx(-0.025, abs=1e-15)
    # the clip is on the norm over the WHOLE structure: two atoms each moving 0.15 clip together (0.212 > 0.2)
    two = FireRef(np.zeros((2, 3)))
    two.step(np.array([[15.0, 0.0, 0.0], [0.0, -15.0, 0.0]]))
    assert np.linalg.norm(two.r) == pytest.approx(0.2, abs=1e-15) and two.r[0, 0] == pytest.approx(-two.r[1, 1], abs=1e-16)


def test_convergence_is_checked_before_stepping():
    ef = well(1.0)
    res = run_ref([[0.05, 0.0, 0.0]], ef, fmax=0.1)  # |F| = 0.05 < fmax: no step, one evaluation
    assert res["n_steps"] == 0 and res["n_evals"] == 1 and res["converged"] and res["r"][0, 0] == 0.05
    res = run_ref([[1.0, 0.0, 0.0]], ef, fmax=0.1, steps=0)  # steps = 0: evaluated once, not converged
    assert res["n_steps"] == 0 and res["n_evals"] == 1 and not res["converged"]
    res = run_ref([[1.0, 0.0, 0.0]], ef, fmax=0.0, steps=7)  # fmax = 0 never converges: exactly `steps` steps
    assert res["n_steps"] == 7 and res["n_evals"] == 8 and not res["converged"]
    res = run_ref([[1.0, 0.0, 0.0]], ef, fmax=1e-3, steps=500)
    assert res["converged"] and abs(res["f"][0, 0]) < 1e-3 and res["n_evals"] == res["n_steps"] + 1
    assert abs(res["r"][0, 0]) < 1e-3


def test_relax_module_exists():
    """The batched relaxer this restatement specifies is part of the package's public surface."""
    import alignn_amd

    assert alignn_amd.relax is relax and set(RelaxResult.__dataclass_fields__) >= {
        "positions", "energies", "forces", "fmax", "converged", "n_steps", "n_evals"}
    with pytest.raises(ValueError):
        relax(None, [np.eye(3)], [np.zeros((1, 3)), np.zeros((1, 3))], forces_fn=lambda lat, pos: None)
    with pytest.raises(TypeError):
        relax(object(), [np.eye(3)], [np.zeros((1, 3))])


def test_relax_validates_before_touching_a_device():
    lat, pos = [np.eye(3) * 5], [np.zeros((2, 3))]
    ff = lambda lat, pos: None  # noqa: E731
    bad = [
        dict(lattices=lat, positions=pos + pos),
        dict(positions=[np.zeros((2, 2))]),
        dict(lattices=[np.eye(3)[:2]]),
        dict(steps=-1),
        dict(fmax=-1.0),
        dict(maxstep=0.0),
        dict(dt=0.0),
    ]
    for kw in bad:
        args = dict(lattices=lat, positions=pos)
        args.update(kw)
        with pytest.raises(ValueError):
            relax(None, args.pop("lattices"), args.pop("positions"), forces_fn=ff, device="cpu", **args)
    with pytest.raises(TypeError):  # a CPU device: the launches are HIP only
        relax(None, lat, pos, forces_fn=ff, device="cpu")
