"""The numpy restatement of the trajectory analysis (tests/traj_ref.py) pinned by properties that need no second implementation:
shell counts of perfect fcc and the pair enumeration of tests/pair_ref.py, ballistic motion, a sine, a known line and the
integral of an exponential.  Then the host-side checks of alignn_amd.trajectory that come before any device work."""

import numpy as np
import pytest

from tests import pair_ref
from tests import traj_ref as ref


def _fcc(a, reps):
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    cells = np.array([[i, j, k] for i in range(reps) for j in range(reps) for k in range(reps)])
    return a * reps * np.eye(3), ((cells[:, None, :] + base[None, :, :]).reshape(-1, 3)) * a


def test_fcc_shells_and_the_pair_enumeration():
    a = 4.0
    C, pos = _fcc(a, 2)  # 32 atoms in an 8 A cube: r_max = 5.2 needs the images of range 1
    n, F, r_max, n_bins = len(pos), 3, 5.2, 26  # dr = 0.2: the shells a / sqrt 2 = 2.83, a = 4.0 and a sqrt(3 / 2) = 4.90 lie
    traj = np.repeat(pos[None], F, axis=0)  #      inside bins 14, 20 (at 0.0 of it: moved below) and 24
    assert ref.image_range(C, r_max) == [1, 1, 1]
    rank, species = ref.groups(None, n)
    # bin edges moved off the shell radii: r_max = 5.3, dr = 5.3 / 26
    r_max = 5.3
    counts, margin, pairs = ref.rdf_counts(traj, C, rank, 1, r_max, n_bins)
    assert margin > 1e-3
    I, J, d, r = pair_ref.pairs(C, pos, r_max)
    assert counts[0].sum() == F * len(I) == pairs and (counts[1] == counts[0]).all()
    g, coord, V, centres = ref.rdf_normalise(counts, C, F, ref.group_counts(rank, 1), r_max)
    assert V == 512.0 and np.allclose(centres[:2], [0.5 * r_max / n_bins, 1.5 * r_max / n_bins], rtol=1e-15)
    dr = r_max / n_bins
    at = lambda radius: coord[0][int(np.floor(radius / dr))]  # the coordination number at the upper edge of the shell's bin
    assert at(a / np.sqrt(2)) == 12.0 and at(a) == 18.0 and at(a * np.sqrt(1.5)) == 42.0  # 12, + 6, + 24
    filled = np.nonzero(counts[0])[0]
    assert list(counts[0][filled]) == [F * n * 12, F * n * 6, F * n * 24]
    # g of a shell: its pairs over the ideal gas's in that bin
    k = filled[0]
    shell = 4 * np.pi / 3 * (((k + 1) * dr) ** 3 - (k * dr) ** 3)
    assert np.isclose(g[0][k], 12 * V / (n * shell), rtol=1e-14)


def test_species_rows_and_both_orders():
    C = np.array([[4.0, 0, 0], [1.3, 3.8, 0], [0.7, -0.9, 4.4]])
    rng = np.random.default_rng(0)
    pos = rng.uniform(0, 1, (7, 3)) @ C
    z = np.array([8, 3, 8, 3, 3, 15, 8])
    rank, species = ref.groups(z, 7)
    assert species == [3, 8, 15] and list(rank) == [2, 1, 2, 1, 1, 3, 2]
    assert list(ref.group_counts(rank, 3)) == [7, 3, 3, 1]
    assert [ref.pair_row(a, b) for a, b in ((1, 1), (1, 2), (2, 2), (1, 3), (2, 3), (3, 3), (3, 1))] == [1, 2, 3, 4, 5, 6, 4]
    assert [ref.row_groups(p) for p in range(7)] == [(0, 0), (1, 1), (1, 2), (2, 2), (1, 3), (2, 3), (3, 3)]
    counts, _, pairs = ref.rdf_counts(pos[None], C, rank, 3, 6.0, 40)
    I, J, d, r = pair_ref.pairs(C, pos, 6.0)
    assert counts[0].sum() == len(I) == pairs and (counts[0] == counts[1:].sum(0)).all()
    for a, b in ((1, 2), (1, 3), (2, 3), (1, 1), (3, 3)):
        both = ((rank[I] == a) & (rank[J] == b)) | ((rank[I] == b) & (rank[J] == a))
        assert counts[ref.pair_row(a, b)].sum() == both.sum()
    # the coordination number of a row a < b counts the b around an a
    g, coord, V, _ = ref.rdf_normalise(counts, C, 1, ref.group_counts(rank, 3), 6.0)
    ab = ((rank[I] == 1) & (rank[J] == 2)).sum()
    assert np.isclose(coord[ref.pair_row(1, 2)][-1], ab / 3.0, rtol=1e-15)
    assert np.isclose(V, abs(np.linalg.det(C)), rtol=1e-14)


def test_ballistic_motion():
    rng = np.random.default_rng(1)
    n, F = 6, 12
    x0 = rng.uniform(0, 5, (n, 3))
    v = np.array([0.25, -0.5, 0.125])  # dyadic: v t is exact
    t = np.arange(F, dtype=np.float64)
    traj = x0[None] + t[:, None, None] * v[None, None, :]
    masses = rng.uniform(1, 50, n)
    rank, _ = ref.groups([3, 3, 8, 8, 8, 3], n)
    with_com, _ = ref.msd(traj, rank, 2, masses, F - 1, remove_com=True)
    assert np.abs(with_com).max() < 1e-24  # the drift is the centre of mass's own
    without, terms = ref.msd(traj, rank, 2, masses, F - 1, remove_com=False)
    want = (t[:, None] * v[None, :]) ** 2
    assert np.abs(without - want[None]).max() <= 1e-13 * want.max()
    assert (terms[0] == n * (F - np.arange(F))).all() and (terms[1] == 3 * (F - np.arange(F))).all()
    strided, terms3 = ref.msd(traj, rank, 2, masses, 4, stride=3, remove_com=False)
    assert np.abs(strided - want[None, :5]).max() <= 1e-13 * want.max()
    assert list(terms3[0]) == [n * ref.n_origins(F, k, 3) for k in range(5)] == [n * m for m in (4, 4, 4, 3, 3)]


def test_sine_vacf_and_vdos_peak():
    n, F, dtau = 4, 400, 2.0  # fs
    f_THz = 5.0
    omega = 2 * np.pi * f_THz * 1e-3  # rad / fs
    t = np.arange(F) * dtau
    amp = np.array([0.1, 0.2, 0.3, 0.4])
    phase = np.array([0.0, 0.7, 1.9, 4.0])
    vx = amp[None, :] * omega * np.cos(omega * t[:, None] + phase[None, :])
    masses = np.array([2.0, 3.0, 5.0, 7.0])
    mom = np.zeros((F, n, 3))
    mom[:, :, 0] = vx * masses[None, :]
    rank, _ = ref.groups(None, n)
    K = 200  # lags: 200 frames = 2 periods of 100 frames; the origins cover whole periods
    C, mag, terms = ref.vacf(mom, rank, 1, masses, K, stride=1)
    assert (mag >= np.abs(C) - 1e-18).all()
    # <cos(wt + p) cos(w(t + tau) + p)> over origins = cos(w tau) / 2 + a term that averages out over whole periods
    norm = C[0] / C[0, 0]
    k = np.arange(K + 1)
    whole = (F - k) % 100 == 0  # lags whose origins span whole periods: the average is exact there
    assert np.abs(norm[whole] - np.cos(omega * k[whole] * dtau)).max() < 1e-12
    assert np.abs(norm - np.cos(omega * k * dtau)).max() < 0.02
    n_freq, f_max = 121, 12.0  # steps of 0.1 THz
    D, scale, nu = ref.vdos(C, dtau, n_freq, f_max, window="hann")
    assert abs(nu[np.argmax(D[0])] - f_THz) <= f_max / (n_freq - 1)
    assert (np.abs(D) <= scale[..., None] * (1 + 1e-12)).all()
    # the transform of the normalised VACF integrates to 1/2 over nu >= 0 (1 over the two-sided axis)
    D2, _, nu2 = ref.vdos(C, dtau, 2001, 250.0, window="hann")  # up to the Nyquist frequency 1 / (2 dtau) = 250 THz
    x = nu2 * 1e-3
    assert abs(float((0.5 * (D2[0][1:] + D2[0][:-1]) * np.diff(x)).sum()) - 0.5) < 1e-3


def test_fit_recovers_a_known_line():
    dtau, K = 0.5, 16
    tau = np.arange(K + 1) * dtau
    slopes, icpts = np.array([0.75, -0.25, 1.5]), np.array([0.5, 2.0, -1.0])  # dyadic: the line's values are exact
    m = icpts[None, :] + tau[:, None] * slopes[None, :]
    out = ref.fit(m[None], dtau, 4, 16)[0]
    assert np.array_equal(out[:3, 0], slopes) and np.array_equal(out[:3, 1], icpts)
    assert out[3, 0] == slopes.sum() and out[3, 1] == icpts.sum()
    assert np.array_equal(out[:, 2], np.zeros(4))  # no residual: no error
    assert np.array_equal(out[:3, 3], slopes / 2) and out[3, 3] == slopes.sum() / 6
    noisy = m + np.random.default_rng(2).normal(0, 0.05, m.shape)
    got = ref.fit(noisy[None], dtau, 2, 16)[0]
    want = np.polyfit(tau[2:], noisy[2:, 1], 1, cov=True)
    assert np.isclose(got[1, 0], want[0][0], rtol=1e-12) and np.isclose(got[1, 1], want[0][1], rtol=1e-12)
    assert np.isclose(got[1, 2], np.sqrt(want[1][0, 0]), rtol=1e-10)


def test_green_kubo_of_a_decaying_exponential():
    dtau, K, tau0, C0 = 1.5, 300, 40.0, 0.02
    k = np.arange(K + 1)
    C = C0 * np.exp(-k * dtau / tau0)
    got = ref.green_kubo(C[None], dtau)[0]
    # the trapezoid of a geometric sequence q^k: (dtau / 2) (1 + q) (1 - q^k) / (1 - q)
    q = np.exp(-dtau / tau0)
    analytic = C0 * 0.5 * (1 + q) * (1 - q ** k) / (1 - q)  # in units of dtau
    want = analytic * dtau * ref.FS * ref.FS / 3.0
    assert got[0] == 0.0 and np.abs(got - want).max() <= 1e-13 * want.max()
    # ... which tends to the integral C0 tau0 / 3 (ASE time units -> A^2 / fs by FS^2)
    assert abs(got[-1] / (C0 * tau0 * ref.FS ** 2 / 3.0) - 1.0) < 2e-3


def test_the_module_exports_and_checks_before_any_device_work():
    import torch

    import alignn_amd
    from alignn_amd import trajectory as tj
    from alignn_amd.dynamics import FS

    assert FS == ref.FS and alignn_amd.A2_FS_TO_CM2_S == tj.A2_FS_TO_CM2_S == 0.1
    for name in ("rdf", "msd", "vacf", "vdos", "diffusion", "green_kubo", "analyze_md", "RDFResult", "MSDResult", "VACFResult",
                 "VDOSResult", "DiffusionResult", "TrajectoryAnalysis"):
        assert getattr(alignn_amd, name) is getattr(tj, name), name
    assert [tj.pair_row(a, b) for a, b in ((0, 0), (1, 1), (2, 1), (2, 2), (1, 3))] == [0, 1, 2, 3, 4]
    assert tj._frames("t", 10, 1, None, 2) == (1, 2, 5) and tj._frames("t", 10, None, None, None) == (0, 1, 10)
    assert tj._frames("t", 10, 8, 3, None)[2] == 0 and tj._frames("t", 10, -4, None, 3) == (6, 3, 2)
    with pytest.raises(ValueError, match="step"):
        tj._frames("t", 10, None, None, 0)
    with pytest.raises(TypeError, match="float64 tensor on the GPU"):
        tj.rdf(torch.zeros(2, 3, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)[None], [3])
    with pytest.raises(ValueError, match="at most 8"):
        tj._groups("t", [9], [np.arange(9)], "cpu")
    ptr, group, count, S, lists = tj._groups("t", [3, 2], [np.array([8, 3, 8]), np.array([1, 1])], "cpu")
    assert S == 2 and lists == [[3, 8], [1]] and group.tolist() == [2, 1, 2, 1, 1] and ptr.tolist() == [0, 3, 5]
    assert count.tolist() == [[3, 1, 2], [2, 2, 0]]

    class NoTrajectory:
        traj_positions = traj_momenta = traj_lattices = None

    with pytest.raises(ValueError, match="trajectory=True"):
        tj.analyze_md(NoTrajectory(), None, [3], None, [np.ones(3)], timestep=1.0)
