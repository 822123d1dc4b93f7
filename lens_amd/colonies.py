"""Colony metrics on the device: connected colonies, mass, area, axes.

The reference's ``colony_metrics_experiment`` wires a ``ColonyShapeDeriver`` into
the lattice (vivarium/compartments/lattice.py:61-64,
vivarium/processes/derive_colony_shape.py:97-217) and emits ``colony_global``:
per colony a surface area, a major and a minor axis, a circumference and a mass,
all taken from an alpha shape of the cell centres.

The definition here is THIS ENGINE'S OWN, not alphashape's (an alpha shape needs
a Delaunay triangulation): no polygon is built and no polygon parity is claimed.

* Two capsules are *linked* when their spines come closer than
  ``width + link_gap`` (the contact kernel's own closest-point arithmetic).
* A *colony* is a connected component of the link graph with at least
  ``min_cells`` members (the reference needs three cells for a polygon).
* ``mass`` is the sum of the members' mass; ``cell_area`` the sum of the
  capsules' own areas (overlaps counted twice) and stands where the reference
  reports the polygon's area; ``major_axis`` / ``minor_axis`` are the colony's
  extents along and across the principal axis of its centres, capsule ends
  included, and stand where the reference takes the sides of the minimum
  rotated rectangle.  There is no ``circumference``: it needs a hull.

On the reference's own seven test scenarios (cells as unit circles,
``link_gap = 0.25``) the colony count and the colony masses are the
reference's.  ``include/vk_kinetics.h`` (vk_colony_metrics) states the
definition and the order of every sum; nothing depends on the storage order.
"""

from __future__ import annotations

import ctypes
import math

from lens_amd import native

TOO_LONG, GAVE_UP = native.VK_COLONIES_TOO_LONG, native.VK_COLONIES_GAVE_UP


class ColonyShapeModel:
    def __init__(self, link_gap: float = 0.5, min_cells: int = 3, max_length: float = 4.0, width: float = 1.0):
        if not (math.isfinite(float(link_gap)) and float(link_gap) >= 0.0):
            raise ValueError('link_gap must be finite and >= 0')
        if int(min_cells) != min_cells or int(min_cells) < 1:
            raise ValueError('min_cells must be an integer >= 1')
        if not float(width) > 0.0:
            raise ValueError('width must be positive')
        if not (math.isfinite(float(max_length)) and float(max_length) >= float(width)):
            raise ValueError('max_length must be finite and at least the width (a disc is the shortest capsule)')
        self.link_gap = float(link_gap)
        self.min_cells = int(min_cells)
        self.max_length = float(max_length)
        self.width = float(width)

    def grid(self, bounds):
        """(gx, gy): the neighbour grid on ``bounds``, cell edges >= max_length + link_gap."""
        return tuple(max(1, int(math.floor(float(b) / (self.max_length + self.link_gap)))) for b in bounds[:2])

    def vk_params(self, bounds, length: float = 2.0, mass: float = 1.0) -> native.VkColoniesParams:
        """``length`` and ``mass``: every agent's where the launch gets no array."""
        p = native.VkColoniesParams()
        p.gx, p.gy = self.grid(bounds)
        p.min_cells = self.min_cells
        p.max_length, p.width, p.link_gap = self.max_length, self.width, self.link_gap
        p.length, p.mass = float(length), float(mass)
        return p


class ColonyMetrics:
    """One result: ``colony`` per agent (-1: in no colony), and per colony
    ``cells``, ``key`` (the smallest member key), ``mass``, ``cell_area``,
    ``centroid`` [C, 2], ``angle``, ``major_axis``, ``minor_axis`` -- numpy
    arrays sliced to the colony count ``n_colonies``."""

    def __init__(self, colony, cells, key, rows):
        self.colony, self.cells, self.key = colony, cells, key
        self.n_colonies = int(cells.shape[0])
        self.rows = rows                      # [VK_COLONY_ROWS, C]: the second moments too
        self.mass = rows[native.VK_COLONY_MASS]
        self.cell_area = rows[native.VK_COLONY_CELL_AREA]
        self.centroid = rows[[native.VK_COLONY_CX, native.VK_COLONY_CY]].T.copy()
        self.angle = rows[native.VK_COLONY_ANGLE]
        self.major_axis = rows[native.VK_COLONY_MAJOR]
        self.minor_axis = rows[native.VK_COLONY_MINOR]

    def as_colony_global(self) -> dict:
        """The reference's emitted ``colony_global`` shape: a list per colony
        under ``surface_area`` (the cell area), ``major_axis``, ``minor_axis``
        and ``mass``.  No ``circumference``."""
        return {'surface_area': self.cell_area.tolist(), 'major_axis': self.major_axis.tolist(),
                'minor_axis': self.minor_axis.tolist(), 'mass': self.mass.tolist()}


class ColonyShape:
    """The scratch and the output tensors of vk_colony_metrics for up to ``ld``
    agents on ``bounds``, allocated once so that a captured graph keeps valid
    pointers.  ``launch`` only launches; ``result`` reads.  ``labels_only`` leaves
    the reductions out (the per-colony values then read NaN)."""

    def __init__(self, model: ColonyShapeModel, bounds, ld: int, device, length: float = 2.0, mass: float = 1.0,
                 labels_only: bool = False):
        import torch
        native.load()
        self.model, self.bounds, self.ld = model, (float(bounds[0]), float(bounds[1])), int(ld)
        self.length, self.mass = float(length), float(mass)
        self.device = native.resolve_device(device)
        dev = self.device
        self.params = model.vk_params(self.bounds, self.length, self.mass)
        self.n = 0
        self.colony = torch.full((self.ld,), -1, dtype=torch.int32, device=dev)
        self.n_colonies = torch.zeros(1, dtype=torch.int32, device=dev)
        self.cells = torch.zeros(self.ld, dtype=torch.int32, device=dev)
        self.colony_key = torch.zeros(self.ld, dtype=torch.int64, device=dev)
        # labels_only: the call ends after the labels, cells and keys (metrics == NULL)
        self.metrics = None if labels_only else torch.zeros((native.VK_COLONY_ROWS, self.ld), dtype=torch.float64,
                                                            device=dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=dev)
        self._bytes = int(native._lib.vk_colonies_scratch_bytes(max(self.ld, 1), self.params.gx * self.params.gy))
        self.scratch = torch.empty(self._bytes + 256, dtype=torch.uint8, device=dev)
        self._off = (-self.scratch.data_ptr()) % 256     # the launch wants a 256-B aligned base

    def launch(self, n: int, location, angle, length=None, mass=None, key=None):
        """Colonies of agents [0, n) of ``location`` [2, ld] (the ``ld`` the buffers
        were made for: it is the stride of the metrics rows too) and ``angle``, on
        the current stream; ``length`` / ``mass`` (float64 rows of at least n
        elements) or the constants, ``key`` (int64 row) or the column index.  The
        flag word is cleared first, so its bits speak of this launch alone.  No
        host read."""
        import torch
        if not (location.dim() == 2 and location.shape[0] == 2 and location.is_contiguous() and
                location.dtype == torch.float64):
            raise ValueError('ColonyShape.launch: location must be a contiguous float64 [2, ld]')
        ld = location.shape[1]
        if ld != self.ld:
            # the launch has one ld: it is also the stride of the metrics rows
            raise ValueError('ColonyShape.launch: location is [2, %d], the buffers were made for ld = %d' % (
                ld, self.ld))
        if not 0 <= n <= ld:
            raise ValueError('ColonyShape.launch: n must lie in [0, ld]')
        for t, dt in ((angle, torch.float64), (length, torch.float64), (mass, torch.float64), (key, torch.int64)):
            if t is not None and not (t.dim() == 1 and t.shape[0] >= n and t.stride(0) == 1 and t.dtype == dt):
                raise ValueError('ColonyShape.launch: angle, length, mass (float64) and key (int64) must be '
                                 'contiguous rows of at least n elements')
        self.flags.zero_()      # on the stream, so a replayed graph clears it too: the bits are this call's
        self.n = int(n)
        native.check(native._lib.vk_colony_metrics(
            ctypes.byref(self.params), n, ld, native.ptr(location), native.ptr(angle), native.ptr(length),
            native.ptr(mass), native.ptr(key), self.bounds[0], self.bounds[1], native.ptr(self.colony),
            native.ptr(self.n_colonies), native.ptr(self.cells), native.ptr(self.colony_key), native.ptr(self.metrics),
            native.ptr(self.flags), self.scratch.data_ptr() + self._off, self._bytes, native.stream_handle()),
            'vk_colony_metrics')

    def check(self):
        """Host read of the flag word: raises on either bit."""
        f = int(self.flags.item())
        if f & GAVE_UP:
            raise native.NativeError('colony metrics: a union gave up after its retry bound; the labels are invalid')
        if f & TOO_LONG:
            raise ValueError('colony metrics: an agent is longer than max_length (the neighbour grid\'s cell edge): '
                             'links may have been missed; build the model with a larger max_length')

    def result(self) -> ColonyMetrics:
        """Reads ``n_colonies`` (a host synchronisation) and the outputs of the
        last launch, sliced to the count."""
        self.check()
        import numpy as np
        c = int(self.n_colonies.item())
        rows = (np.full((native.VK_COLONY_ROWS, c), np.nan) if self.metrics is None      # labels only
                else self.metrics[:, :c].cpu().numpy())
        return ColonyMetrics(self.colony[:self.n].cpu().numpy(), self.cells[:c].cpu().numpy(),
                             self.colony_key[:c].cpu().numpy(), rows)
