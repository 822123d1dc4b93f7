"""Colony mechanics: growing capsules push each other apart on the device.

The reference resolves overlapping cells with its ``multibody`` process
(vivarium/processes/multibody_physics.py), a pymunk rigid-body simulation.
This engine has no pymunk and does not imitate its impulse solver: the contact
model here is THIS ENGINE'S OWN and no parity with pymunk trajectories is
claimed.  What stays the reference's is everything that feeds it -- the
capsule length and width DeriveGlobals computes, the growth that lengthens a
cell, the daughter placement of division.

:class:`ContactModel` holds the constants of a Jacobi relaxation of capsule
overlaps (vk_contact_step, lens_amd/csrc/vk_contact.hip states every formula):
per iteration every agent is pushed by ``0.5 * stiffness`` of each overlap
along the contact normal and turned by that push's moment about its centre
times ``12 / L^2`` (the rotational-to-translational mobility ratio of a
uniformly dragged rod); the summed push is capped at ``max_push``, the turn at
``max_turn``; optional Gaussian ``jitter`` (what lets an exactly collinear
lineage buckle into two dimensions -- the reference has ``jitter_force`` for
the same reason); the centre is clamped into the lattice bounds.

A ``Colony(..., mechanics=model)`` runs the launch first in every step and
re-bins its agents on the device, as a motile colony does.  With ``cells=`` a
capsule's length is the agent's ``VK_CELL_LENGTH`` row and its angle the
``VK_CELL_ANGLE`` row; without, every agent has ``length`` and the colony owns
a ``mech_angle`` array.

``channels=`` turns the plane into the reference's mother machine
(vivarium/library/pymunk_multibody.py:218-230, multibody_physics.py:232-250):
vertical lines at ``x = channel_space * l``, ``l = 0 .. n_lines - 1``, from the
floor up to ``channel_height``, of thickness ``spacer_thickness``.  The launch
(vk_contact_step_channels) keeps every agent below ``channel_height`` in the
channel it is in -- a projection of its angle and centre, this engine's own wall
law, no pymunk segments and no flow -- and flags the agents above it, which the
colony removes at the end of the step.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from lens_amd import native

TOO_LONG = 1      # bit 0 of the flag word
CHANNEL_KEYS = ('channel_height', 'channel_space', 'spacer_thickness')


class ContactModel:
    def __init__(self, iterations: int = 4, stiffness: float = 0.5, max_length: float = 4.0, width: float = 1.0,
                 length: float = 2.0, max_push: Optional[float] = None, max_turn: float = 0.5, jitter: float = 0.0,
                 jitter_angle: float = 0.0, seed: int = 0, angles=None, channels=None, **unknown):
        if unknown:
            raise ValueError('unknown ContactModel parameters: %s' % sorted(unknown))
        if int(iterations) != iterations or int(iterations) < 1:
            raise ValueError('iterations must be an integer >= 1')
        if not (0.0 < float(stiffness) <= 1.0):
            raise ValueError('stiffness must lie in (0, 1]')
        if not float(width) > 0.0:
            raise ValueError('width must be positive')
        if not float(max_length) >= float(width):
            raise ValueError('max_length must be at least the width (a disc is the shortest capsule)')
        if not float(length) > 0.0:
            raise ValueError('length must be positive')
        if max_push is not None and not float(max_push) >= 0.0:
            raise ValueError('max_push must be >= 0')
        if not float(max_turn) >= 0.0:
            raise ValueError('max_turn must be >= 0')
        if not (float(jitter) >= 0.0 and float(jitter_angle) >= 0.0):
            raise ValueError('jitter and jitter_angle must be >= 0')
        self.iterations = int(iterations)
        self.stiffness = float(stiffness)
        self.max_length = float(max_length)
        self.width = float(width)
        self.length = float(length)
        self.max_push = self.width / 2 if max_push is None else float(max_push)
        self.max_turn = float(max_turn)
        self.jitter, self.jitter_angle = float(jitter), float(jitter_angle)
        self.seed = int(seed)
        self.angles = angles                 # initial axis angles (rad) per agent; None: seeded uniform
        self.channels = None
        if channels is not None:
            # the reference's multibody keys (its 'mother_machine' dictionary)
            ch = dict(channels)
            bad = sorted(set(ch) - set(CHANNEL_KEYS))
            if bad:
                raise ValueError('unknown channels keys: %s (known: %s)' % (bad, list(CHANNEL_KEYS)))
            for k in ('channel_height', 'channel_space'):
                if k not in ch:
                    raise ValueError('channels needs %r' % k)
            ch.setdefault('spacer_thickness', 0.1)
            ch = {k: float(ch[k]) for k in CHANNEL_KEYS}
            if not ch['channel_height'] > 0.0:
                raise ValueError('channels: channel_height must be positive')
            if not ch['spacer_thickness'] >= 0.0:
                raise ValueError('channels: spacer_thickness must be >= 0')
            if not ch['channel_space'] >= self.width + 2.0 * ch['spacer_thickness']:
                raise ValueError('channels: channel_space must be at least width + 2 * spacer_thickness '
                                 '(a cell must fit between two lines)')
            self.channels = ch

    def grid(self, bounds):
        """(gx, gy): the neighbour grid on ``bounds``, cell edges >= max_length."""
        return tuple(max(1, int(math.floor(float(b) / self.max_length))) for b in bounds[:2])

    def initial_angles(self, n: int, ld: int, angles=None) -> np.ndarray:
        """mech_angle[ld]: ``angles``, or uniform in [0, 2 pi) from a numpy
        generator seeded with the model's seed (as MotilityModel.initial_rows)."""
        out = np.zeros(ld)
        if angles is None:
            angles = self.angles
        if angles is None:
            angles = np.random.default_rng(self.seed).uniform(0.0, 2.0 * math.pi, n)
        angles = np.asarray(angles, dtype=np.float64)
        if angles.shape[0] < n:
            raise ValueError('angles must give every agent an axis angle (%d < %d)' % (angles.shape[0], n))
        out[:n] = angles[:n]
        return out

    def vk_params(self, bounds) -> native.VkContactParams:
        p = native.VkContactParams()
        p.iterations = self.iterations
        p.gx, p.gy = self.grid(bounds)
        for name in ('stiffness', 'max_length', 'width', 'length', 'max_push', 'max_turn', 'jitter', 'jitter_angle'):
            setattr(p, name, getattr(self, name))
        p.seed = self.seed & (2 ** 64 - 1)
        return p

    def n_lines(self, bounds) -> int:
        """floor(bound_x / channel_space): the reference's count of wall lines."""
        return int(math.floor(float(bounds[0]) / self.channels['channel_space']))

    def check_channels(self, bounds):
        """The channels against a plane of ``bounds``: raises ValueError."""
        ch = self.channels
        if not ch['channel_height'] <= float(bounds[1]):
            raise ValueError('channels: channel_height (%r) must not exceed bound_y (%r)' % (
                ch['channel_height'], float(bounds[1])))
        if self.n_lines(bounds) < 1:
            raise ValueError('channels: channel_space (%r) leaves no line on bound_x (%r)' % (
                ch['channel_space'], float(bounds[0])))

    def vk_channels(self, bounds) -> Optional[native.VkContactChannels]:
        if self.channels is None:
            return None
        self.check_channels(bounds)
        c = native.VkContactChannels()
        c.height, c.space = self.channels['channel_height'], self.channels['channel_space']
        c.spacer = self.channels['spacer_thickness']
        c.n_lines = self.n_lines(bounds)
        return c


class ContactBuffers:
    """What vk_contact_step needs beside the agents, for up to ``ld`` agents on
    a grid of ``n_grid_cells``: the scratch, the iteration counter (the Philox
    counter word, advanced by every launch) and the flag word.  Allocated once,
    so that a captured graph keeps valid pointers."""

    def __init__(self, ld: int, n_grid_cells: int, device, counter: int = 0):
        import torch
        self.ld, self.n_grid_cells = int(ld), int(n_grid_cells)
        self.counter = torch.full((1,), int(counter), dtype=torch.int64, device=device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=device)
        nbytes = int(native._lib.vk_contact_scratch_bytes(max(self.ld, 1), self.n_grid_cells))
        self.scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
        self._off = (-self.scratch.data_ptr()) % 256     # the launch wants a 256-B aligned base
        self._bytes = nbytes

    def check(self):
        """Host read of the flag word: raises when an agent outgrew the grid."""
        if int(self.flags.item()) & TOO_LONG:
            raise ValueError('mechanics: an agent is longer than max_length (the neighbour grid\'s cell edge): '
                             'contacts may have been missed; build the ContactModel with a larger max_length')


def contact_step(model: ContactModel, lattice, location, angle, n: int, buffers: ContactBuffers, length=None,
                 key=None, bin_lin=None, bin_ix=None, outflow=None):
    """One vk_contact_step launch sequence on the current stream:
    ``model.iterations`` relaxation iterations for agents [0, n) of ``location``
    [2, ld] and ``angle`` [ld] (both updated in place); ``length`` [ld] or None
    for the model's constant.  ``bin_lin`` / ``bin_ix`` (int32 [ld]) receive the
    bins.  A model with channels goes through vk_contact_step_channels, and
    ``outflow`` (int32 [ld], optional) receives 1 for every agent above the channels
    after an iteration, 0 for the others.  The lattice must hold whole, unbanded
    planes.  No host read."""
    import torch
    from lens_amd.lattice import whole_plane
    if not whole_plane(lattice):
        raise ValueError('contact_step: a whole, unbanded plane')
    ld = location.shape[1]
    for t in (angle, length):
        if t is not None and not (t.dim() == 1 and t.shape[0] == ld and t.stride(0) == 1):
            raise ValueError('contact_step: angle and length must be rows of ld elements beside location [2, ld]')
    if not location.is_contiguous():
        raise ValueError('contact_step: location must be contiguous')
    p = model.vk_params(lattice.bounds)
    if n > buffers.ld or p.gx * p.gy != buffers.n_grid_cells:
        raise ValueError('contact_step: the buffers were sized for fewer agents or another grid')
    if bin_lin is None:
        bin_lin = torch.zeros(ld, dtype=torch.int32, device=location.device)
    ch = model.vk_channels(lattice.bounds)
    if ch is not None:
        if outflow is not None and not (outflow.dtype == torch.int32 and outflow.dim() == 1 and
                                        outflow.shape[0] >= ld and outflow.stride(0) == 1):
            raise ValueError('contact_step: outflow must be an int32 row of ld elements')
        native.check(native._lib.vk_contact_step_channels(
            ctypes.byref(p), n, ld, native.ptr(location), native.ptr(angle), native.ptr(length), native.ptr(key),
            native.ptr(buffers.counter), native.ptr(buffers.flags), lattice.n_bins[0], lattice.n_bins[1],
            lattice.bounds[0], lattice.bounds[1], native.ptr(bin_lin), native.ptr(bin_ix),
            buffers.scratch.data_ptr() + buffers._off, buffers._bytes, ctypes.byref(ch), native.ptr(outflow),
            native.stream_handle()), 'vk_contact_step_channels')
        return bin_lin
    if outflow is not None:
        raise ValueError('contact_step: outflow needs a model with channels')
    native.check(native._lib.vk_contact_step(
        ctypes.byref(p), n, ld, native.ptr(location), native.ptr(angle), native.ptr(length), native.ptr(key),
        native.ptr(buffers.counter), native.ptr(buffers.flags), lattice.n_bins[0], lattice.n_bins[1],
        lattice.bounds[0], lattice.bounds[1], native.ptr(bin_lin), native.ptr(bin_ix),
        buffers.scratch.data_ptr() + buffers._off, buffers._bytes, native.stream_handle()), 'vk_contact_step')
    return bin_lin
