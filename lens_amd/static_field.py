"""Static fields: analytic gradients, evaluated on the device.

The reference's chemotaxis experiment (vivarium/experiments/chemotaxis.py) runs on a
``StaticField`` deriver (vivarium/processes/static_field.py:25-119), not on a diffusing
lattice: a gaussian, linear or exponential function of the distance from a centre, evaluated
at every agent's continuous location after every update.  ``make_gradient``
(vivarium/processes/diffusion_field.py:42-206) fills a lattice's initial planes with the same
functions at the middle of every bin.  Both are one device function here
(``lens_amd/csrc/vk_gradient.h``), in the reference's operation order:

* :class:`StaticField` -- the model, an environment of :class:`lens_amd.colony.Colony`;
* :func:`make_gradient` -- the initial planes (``vk_gradient_fill``);
* :func:`static_gather` -- the field at agents' locations (``vk_static_gather``).

The field arithmetic is the reference's.  What moves the agents through it is not
(:mod:`lens_amd.motility`).
"""

from __future__ import annotations

import ctypes
import math
from typing import Sequence

from lens_amd import native

TYPES = {'uniform': native.VK_GRADIENT_UNIFORM, 'gaussian': native.VK_GRADIENT_GAUSSIAN,
         'linear': native.VK_GRADIENT_LINEAR, 'exponential': native.VK_GRADIENT_EXPONENTIAL}


def gradient_specs(gradient, bounds, static: bool = False):
    """``(molecules, [VkGradientSpec])`` of a reference ``gradient`` dict over ``bounds``.

    The centre is multiplied by the bounds here, in Python doubles, as the reference does.
    Defaults are the reference's: ``base`` 0.0 for linear, ``scale`` 1 for exponential.
    ``static``: the rules of the ``StaticField`` deriver, which has no uniform type."""
    kind = gradient.get('type')
    if kind not in TYPES:
        raise ValueError('unknown gradient type %r (one of %s)' % (kind, sorted(TYPES)))
    if static and kind == 'uniform':
        raise ValueError("a static field cannot be 'uniform': the reference's StaticField returns nothing for it")
    molecules, specs = [], []
    for mol, s in gradient.get('molecules', {}).items():
        g = native.VkGradientSpec()
        g.type = TYPES[kind]
        if kind == 'uniform':
            g.p0 = float(s)
        else:
            g.cx = s['center'][0] * bounds[0]
            g.cy = s['center'][1] * bounds[1]
            if kind == 'gaussian':
                g.p0 = float(s['deviation'])
                if g.p0 == 0.0:
                    raise ValueError('gradient of %s: a zero deviation divides by zero' % mol)
            elif kind == 'linear':
                g.p0, g.p1 = float(s.get('base', 0.0)), float(s['slope'])
            else:
                g.p0, g.p1 = float(s['base']), float(s.get('scale', 1))
                if not g.p0 > 0.0:
                    raise ValueError('gradient of %s: an exponential base must be positive (got %r): '
                                     'base ** distance would be complex' % (mol, s['base']))
        molecules.append(mol)
        specs.append(g)
    return molecules, specs


def _spec_array(specs):
    arr = (native.VkGradientSpec * max(len(specs), 1))()
    for i, g in enumerate(specs):
        arr[i] = g
    return arr


def host_value(g, x: float, y: float) -> float:
    """One spec at one point on the host, in the device function's operation order."""
    if g.type == native.VK_GRADIENT_UNIFORM:
        return g.p0
    dx, dy = x - g.cx, y - g.cy
    d = math.sqrt(dx * dx + dy * dy) / 1000.0
    if g.type == native.VK_GRADIENT_GAUSSIAN:
        return math.exp((-(d * d)) / (2.0 * (g.p0 * g.p0)))
    if g.type == native.VK_GRADIENT_LINEAR:
        return g.p0 + g.p1 * d
    return g.p1 * g.p0 ** d


class StaticField:
    """The reference's ``StaticField`` configuration: ``molecules``, ``bounds`` and a
    ``gradient`` of ``{'type', 'molecules': {mol: {center, deviation | base, slope | base, scale}}}``.

    Molecules listed but absent from the gradient are never written (the reference's update
    holds only the gradient's molecules); a linear field that goes negative is passed on as it
    is.  ``n_bins`` only gives the bins that motile agents emit."""

    def __init__(self, molecules: Sequence[str], bounds, gradient, n_bins=(10, 10)):
        self.molecules = list(molecules)
        self.bounds = [float(bounds[0]), float(bounds[1])]
        self.n_bins = [int(n_bins[0]), int(n_bins[1])]
        if not (self.bounds[0] > 0.0 and self.bounds[1] > 0.0 and self.n_bins[0] > 0 and self.n_bins[1] > 0):
            raise ValueError('bounds and n_bins must be positive')
        self.gradient = gradient
        self.gradient_molecules, self._specs = gradient_specs(gradient, bounds, static=True)
        for m in self.gradient_molecules:
            if m not in self.molecules:
                raise ValueError('gradient molecule %r is not one of the molecules %r' % (m, self.molecules))

    def spec(self, molecule):
        if molecule not in self.gradient_molecules:
            raise ValueError('%r has no gradient (gradient molecules: %r)' % (molecule, self.gradient_molecules))
        return self._specs[self.gradient_molecules.index(molecule)]

    def specs(self):
        """The ctypes array of ``vk_gradient_spec``, in the gradient's molecule order."""
        return _spec_array(self._specs)

    def value(self, molecule, x: float, y: float) -> float:
        """The field of ``molecule`` at one point, on the host (an ``initial_ligand``)."""
        return host_value(self.spec(molecule), float(x), float(y))

    def gather(self, loc, n: int, conc, rows):
        """``conc[rows[m]]`` of the first ``n`` agents := the field of molecule ``m`` at ``loc``
        ([2, ld]); ``rows`` maps gradient molecules to rows of ``conc``."""
        static_gather(self._specs, [(self.gradient_molecules.index(m), r) for m, r in rows.items()], loc, n, conc)


def make_gradient(gradient, n_bins, bounds, device=None):
    """``{molecule: [nx, ny] tensor}``: the reference's ``make_gradient`` on the device, all
    four types (one ``vk_gradient_fill`` per ``VK_GRADIENT_MAX`` molecules)."""
    import torch
    lib = native.load()
    device = native.resolve_device(device)
    nx, ny = int(n_bins[0]), int(n_bins[1])
    molecules, specs = gradient_specs(gradient, bounds)
    planes = torch.empty((max(len(specs), 1), nx, ny), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        for i in range(0, len(specs), native.VK_GRADIENT_MAX):
            chunk = specs[i:i + native.VK_GRADIENT_MAX]
            native.check(lib.vk_gradient_fill(_spec_array(chunk), len(chunk), native.ptr(planes[i]), nx * ny, ny,
                                              nx, ny, float(bounds[0]), float(bounds[1]), native.stream_handle()),
                         'vk_gradient_fill')
    return {m: planes[f] for f, m in enumerate(molecules)}


def static_gather(specs, field_rows, loc, n: int, conc):
    """``conc[row, a] = specs[field]`` at ``(loc[0, a], loc[1, a])`` for every ``(field, row)`` of
    ``field_rows`` and ``a < n`` (``vk_static_gather``, ``VK_GRADIENT_MAX`` map entries per
    launch).  Columns at and beyond ``n`` and rows not named are left alone."""
    lib = native.load()
    if loc.dim() != 2 or loc.shape[0] != 2 or conc.dim() != 2 or loc.stride(1) != 1 or conc.stride(1) != 1:
        raise ValueError('loc must be [2, ld] and conc [rows, ld_conc], both with unit column stride')
    if not 0 <= n <= min(loc.shape[1], conc.shape[1]):
        raise ValueError('n = %d agents do not fit loc / conc' % n)
    field_rows = list(field_rows)
    for f, r in field_rows:
        if not (0 <= f < len(specs) and 0 <= r < conc.shape[0]):
            raise ValueError('map entry (%d, %d) outside the specs / the rows of conc' % (f, r))
    for i in range(0, len(field_rows), native.VK_GRADIENT_MAX):
        chunk = field_rows[i:i + native.VK_GRADIENT_MAX]
        used = [specs[f] for f, _ in chunk]                   # a chunk's specs, renumbered 0..
        field_of = (ctypes.c_int32 * len(chunk))(*range(len(chunk)))
        row_of = (ctypes.c_int32 * len(chunk))(*[r for _, r in chunk])
        native.check(lib.vk_static_gather(_spec_array(used), field_of, row_of, len(chunk), native.ptr(loc),
                                          loc.stride(0), n, native.ptr(conc), conc.stride(0),
                                          native.stream_handle()), 'vk_static_gather')
