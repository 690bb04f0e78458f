"""What the batched drivers (``relax``, ``run_md``, ``phonons``) share: the checks of their inputs, the packing of B crystals
on the device, and the force evaluation - the reference's ``AlignnAtomwiseCalculator`` (alignn/ff/calculators.py:280-370) for
a batch of structures.

The inputs: ``lattices`` B cells [3, 3] (rows a, b, c), ``positions`` B Cartesian [n_i, 3], ``atom_features`` B [n_i, F] (the
model's ``atom_input_features``), and where a driver takes them ``masses`` B [n_i] in amu (finite, > 0).

The model: an ``ALIGNNAtomWise`` with ``calculate_gradient=True`` in eval mode.  One evaluation builds the graph batch of its
structures (``neighbors.crystal_batch`` with ``cutoff``, ``max_neighbors``, ``neighbor_strategy``; the line graph only when the
model has ALIGNN layers) and applies the calculator's rules, in float32 and then as float64: energies ``out * n_i`` when
``intensive`` (else ``out``), forces ``grad * force_multiplier``, and where a driver needs them the per-crystal stresses
(``stresswise_weight != 0``, ``batch_stress=True``) as ``sym(stress) * stress_weight / 160.21766208`` in eV/A^3 (the
calculator's ``stress_wt``, 1.0 in ``ForceField``).

``forces_fn(lattices, positions) -> (energy [B'], forces [sum n_i, 3])`` replaces the model: it gets the cells [3, 3] and the
Cartesian positions [n_i, 3] of the B' structures of one evaluation (lists of device tensors, not to be modified) and returns
their energies and concatenated forces as they are to be used (no multiplier applied); where a driver needs stresses it
returns ``(energy, forces, stress [B', 3, 3])``, the stress in eV/A^3 with ASE's sign (d E / d strain / volume), used as given.

Every driver runs on the GPU: the model's device, else ``device``, else the current one.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import neighbors

EV_A3_TO_GPA = 160.21766208  # eV/A^3 -> GPa (ASE 3.22's 1e24 / kJ): the calculator's stress unit


def shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def check_inputs(who: str, model, lattices: Sequence, positions: Sequence, atom_features: Optional[Sequence],
                 masses: Optional[Sequence] = None, *, forces_fn: Optional[Callable] = None,
                 stress: bool = False) -> List[int]:
    """The host-side checks of a driver's structures and model, before any device work; returns the atom counts n_i.
    ``who`` prefixes the messages; ``masses`` only for the drivers that take them; ``stress``: the model must predict
    per-crystal stresses."""
    B = len(positions)
    if B == 0 or len(lattices) != B or (masses is not None and len(masses) != B):
        counts = f"{len(lattices)} lattices, {B} position arrays" + ("" if masses is None else f", {len(masses)} mass arrays")
        raise ValueError(f"{who}: {counts} (need the same number, at least one)")
    ns = []
    for i, p in enumerate(positions):
        sh = shape_of(p)
        if len(sh) != 2 or sh[1] != 3 or sh[0] < 1:
            raise ValueError(f"{who}: positions[{i}] is {sh}, need [n_i, 3] with n_i >= 1")
        ns.append(int(sh[0]))
    for i, lat in enumerate(lattices):
        if shape_of(lat) != (3, 3):
            raise ValueError(f"{who}: lattices[{i}] is {shape_of(lat)}, need [3, 3]")
    if masses is not None:
        for i, m in enumerate(masses):
            if shape_of(m) != (ns[i],):
                raise ValueError(f"{who}: masses[{i}] is {shape_of(m)}, need [{ns[i]}]")
        mass = _host_masses(masses)
        if not bool(torch.isfinite(mass).all()) or not bool((mass > 0).all()):
            raise ValueError(f"{who}: masses must be finite and > 0")
    if forces_fn is None:
        from .alignn_atomwise import ALIGNNAtomWise

        if not isinstance(model, ALIGNNAtomWise):
            raise TypeError(f"{who}: the model must be an ALIGNNAtomWise, got {type(model).__name__} (or pass forces_fn)")
        if not model.config.calculate_gradient:
            raise ValueError(f"{who}: the model has calculate_gradient=False and predicts no forces")
        if model.training:
            raise ValueError(f"{who}: the model is in training mode; call model.eval() first")
        if stress and (model.config.stresswise_weight == 0 or not model.config.batch_stress):
            raise ValueError(f"{who}: the model must predict per-crystal stresses: stresswise_weight != 0 and "
                             "batch_stress=True")
        if atom_features is None or len(atom_features) != B:
            raise ValueError(f"{who}: the model needs atom_features, one [n_i, F] array per structure")
        F_in = model.config.atom_input_features
        for i, f in enumerate(atom_features):
            if shape_of(f) != (ns[i], F_in):
                raise ValueError(f"{who}: atom_features[{i}] is {shape_of(f)}, need [{ns[i]}, {F_in}]")
    return ns


def gpu_device(who: str, model, forces_fn: Optional[Callable], device) -> torch.device:
    """The device a driver runs on (the model's, else ``device``, else the current one); a ``TypeError`` if it is not a GPU.
    Called after every ``ValueError`` check of the driver."""
    if forces_fn is None:
        dev = model.fc.weight.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise TypeError(f"{who} runs on the GPU (its launches are HIP only), got device {dev}")
    return dev


def _host_masses(masses: Sequence) -> torch.Tensor:
    return torch.cat([torch.as_tensor(m).detach().to("cpu", torch.float64).reshape(-1) for m in masses])


@dataclass
class Packed:
    """B structures on the device in the layout the kernels take."""

    lat: torch.Tensor  # [B, 3, 3] float64
    pos: torch.Tensor  # [N, 3] float64, Cartesian, the structures' rows one after the other
    ptr: List[int]  # [B + 1] host prefix sums of the n_i
    atom_ptr: torch.Tensor  # [B + 1] int32, the same on the device
    inv: Optional[torch.Tensor] = None  # [B, 3, 3] float64, inverse cells (``frac=True``)
    frac: Optional[torch.Tensor] = None  # [N, 3] float64, fractional coordinates wrapped into [0, 1) (``frac=True``)
    mass: Optional[torch.Tensor] = None  # [N] float64, amu (``masses`` given)

    def rows(self, t: torch.Tensor) -> List[torch.Tensor]:
        """The per-structure views of the rows of ``t`` [N, ...]."""
        return [t[self.ptr[s]:self.ptr[s + 1]] for s in range(len(self.ptr) - 1)]


def pack(lattices: Sequence, positions: Sequence, ns: List[int], dev: torch.device, masses: Optional[Sequence] = None,
         frac: bool = True) -> Packed:
    """Stack the cells and concatenate the positions (and masses) of checked inputs on ``dev``; with ``frac``, the inverse
    cells and the wrapped fractional coordinates too."""
    lat = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices])
    pos = torch.cat([torch.as_tensor(p).to(dev, torch.float64) for p in positions]).contiguous()
    ptr = [0]
    for n in ns:
        ptr.append(ptr[-1] + n)
    out = Packed(lat=lat, pos=pos, ptr=ptr, atom_ptr=torch.tensor(ptr, dtype=torch.int32, device=dev))
    if masses is not None:
        out.mass = _host_masses(masses).to(dev)
    if frac:
        out.inv = torch.linalg.inv(lat).contiguous()
        site = torch.repeat_interleave(torch.arange(len(ns), device=dev), torch.tensor(ns, device=dev))
        f = torch.bmm(pos.unsqueeze(1), out.inv[site]).squeeze(1)
        f = f - torch.floor(f)
        out.frac = torch.where(f < 1.0, f, torch.zeros_like(f)).contiguous()
    return out


class ForceEvaluator:
    """Energies, forces and (with ``stress_weight``) stresses of a list of structures, through the model or ``forces_fn``
    (the module docstring), as contiguous float64 device tensors.  ``atom_features`` and ``counts`` are per structure
    index: a call names the structures it evaluates by these indices.  ``replay``: the model through
    ``md.GraphedForceField`` (the same bits).  ``energies=False``: the energies are not used; a call returns None for
    them."""

    def __init__(self, who: str, model, forces_fn: Optional[Callable], atom_features: Optional[Sequence], counts: List[int],
                 dev: torch.device, *, cutoff: float, max_neighbors: int, neighbor_strategy: str, intensive: bool,
                 force_multiplier: float, stress_weight: Optional[float] = None, replay: bool = False,
                 energies: bool = True):
        self.who, self.forces_fn, self.counts, self.dev, self.energies = who, forces_fn, counts, dev, energies
        self.intensive, self.force_multiplier, self.stress_weight = intensive, force_multiplier, stress_weight
        self._which = self._rows = self._n = None
        if forces_fn is None:
            self.feats = [torch.as_tensor(f).to(dev, torch.float32) for f in atom_features]
            self.graph = dict(device=dev, cutoff=cutoff, max_neighbors=max_neighbors, line_graph=len(model.alignn_layers) > 0,
                              neighbor_strategy=neighbor_strategy)
            if replay:
                from .md import GraphedForceField

                model = GraphedForceField(model)
            self.model = model

    def __call__(self, which: Sequence[int], lattices: List[torch.Tensor], frac: List[torch.Tensor],
                 cart: Optional[List[torch.Tensor]]):
        """(energy [B'], forces [sum n_i, 3], stress [B', 3, 3] or None) of the structures ``which`` with cells
        ``lattices``: the model reads their wrapped fractional coordinates ``frac``, ``forces_fn`` their Cartesian
        positions ``cart``."""
        if which != self._which:  # (a new set of structures: the n_i copy to the device comes before the step's work)
            self._which, self._rows = list(which), sum(self.counts[s] for s in which)
            if self.forces_fn is None and self.energies and self.intensive:
                self._n = torch.tensor([self.counts[s] for s in which], dtype=torch.float32, device=self.dev)
        energy = stress = None
        if self.forces_fn is None:
            batch = neighbors.crystal_batch(lattices, frac, atom_features=[self.feats[s] for s in which], **self.graph)
            with torch.enable_grad():  # (the force head differentiates the energy)
                res = self.model(batch)
            if self.energies:
                out = res["out"].detach().reshape(-1).float()
                energy = ((out * self._n) if self.intensive else out).double()
            forces = (res["grad"].detach().reshape(-1, 3) * self.force_multiplier).double()
            if self.stress_weight is not None:  # the calculator: voigt (symmetrised) stress * stress_wt / 160.21766208, float32
                st = res["stresses"].detach().reshape(-1, 3, 3).float()
                stress = ((st + st.transpose(1, 2)) / 2 * self.stress_weight / EV_A3_TO_GPA).double()
        else:
            out = self.forces_fn(lattices, cart)
            if self.stress_weight is not None:
                if not isinstance(out, (tuple, list)) or len(out) != 3:
                    raise ValueError(f"{self.who}: forces_fn must return (energy, forces, stress) when stresses are used")
                energy, forces, stress = out
                stress = torch.as_tensor(stress).to(self.dev, torch.float64)
            else:
                energy, forces = out
            energy = torch.as_tensor(energy).to(self.dev, torch.float64).reshape(-1) if self.energies else None
            forces = torch.as_tensor(forces).to(self.dev, torch.float64).reshape(-1, 3)
        if (energy is not None and energy.numel() != len(which)) or forces.shape[0] != self._rows:
            got = "" if energy is None else f"{energy.numel()} energies / "
            raise ValueError(f"{self.who}: evaluation returned {got}{forces.shape[0]} force rows for {len(which)} structures / "
                             f"{self._rows} atoms")
        if stress is not None:
            if stress.shape != (len(which), 3, 3):
                raise ValueError(f"{self.who}: evaluation returned stresses of shape {tuple(stress.shape)} for {len(which)} "
                                 "structures")
            stress = stress.contiguous()
        return None if energy is None else energy.contiguous(), forces.contiguous(), stress
