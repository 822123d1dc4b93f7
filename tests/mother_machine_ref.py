"""NumPy restatement of the mother machine for the tests: the population plan
(vk_population_plan), the channel projection and the outflow flag of
vk_contact_step_channels, and a whole colony of growing, dividing cells in
channels built from them.  The capped push and the jitter are mechanics_ref's
(imported, not copied); the operations of the projection are written in the
kernel's order (lens_amd/csrc/vk_contact.hip), so the two differ only through
cos / sin / atan2 of the device library against libm.
"""

import math

import numpy as np

import mechanics_ref as ref


# ---------------------------------------------------------------------------
# population plan
# ---------------------------------------------------------------------------

def plan(divide, remove, n):
    """(src_index, kind, n_out) of vk_population_plan; either flag array may be None."""
    d = np.zeros(n, dtype=bool) if divide is None else np.asarray(divide[:n]) != 0
    r = np.zeros(n, dtype=bool) if remove is None else np.asarray(remove[:n]) != 0
    keep = np.nonzero(~r & ~d)[0]
    mothers = np.nonzero(d & ~r)[0]
    src = np.concatenate([keep, np.repeat(mothers, 2)]).astype(np.int32)
    kind = np.concatenate([np.full(len(keep), -1), np.tile([0, 1], len(mothers))]).astype(np.int32)
    return src, kind, int(n - r.sum() + len(mothers))


# ---------------------------------------------------------------------------
# channel projection and outflow flag
# ---------------------------------------------------------------------------

def n_lines(bounds, space):
    return int(math.floor(bounds[0] / space))


def channel_of(x, bounds, space):
    """clamp(floor(x / space), 0, n_lines - 1)"""
    return np.clip(np.floor(x / space), 0, n_lines(bounds, space) - 1).astype(np.int64)


def project(x_snap, x, y, th, L, bounds, *, width, height, space, spacer):
    """The wall law on moved (x, y, theta), before the plane's clamp: new (x, theta)
    and the outflow flags.  ``x_snap``: the centres before the move."""
    r = width / 2.0
    h = np.maximum(L - width, 0.0) / 2.0
    out = y > height
    c = channel_of(x_snap, bounds, space)
    lo = c * space + (r + spacer)
    hi = np.where(c + 1 < n_lines(bounds, space), (c + 1) * space - (r + spacer), np.nextafter(bounds[0], 0.0))
    cs, sn = np.cos(th), np.sin(th)
    with np.errstate(divide='ignore', invalid='ignore'):
        cmax = np.minimum((hi - lo) / (2.0 * h), 1.0)
    ac = np.abs(cs)
    turn = (h > 0.0) & (ac > cmax)
    cm = np.where(turn, cmax, 0.0)
    th_new = np.where(turn, np.arctan2(np.copysign(np.sqrt(1.0 - cm * cm), sn), np.copysign(cm, cs)), th)
    ac = np.where(h > 0.0, np.where(turn, cmax, ac), 0.0)
    e = h * ac
    x_new = np.minimum(np.maximum(x, lo + e), np.maximum(hi - e, lo + e))
    return np.where(out, x, x_new), np.where(out, th, th_new), out


def iterate(x, y, th, L, keys, bounds, s_global, channels, info=None, **kw):
    """One iteration with channels: mechanics_ref's push and jitter, the projection,
    the plane's clamp.  Returns (x, y, theta, outflow).  ``info`` also receives
    'height_margin', the smallest |y - height| of the moved centres."""
    mx, my, mth = ref.iterate(x, y, th, L, keys, bounds, s_global, clamp=False, info=info, **kw)
    px, pth, out = project(x, mx, my, mth, L, bounds, width=kw.get('width', 1.0), height=channels['height'],
                           space=channels['space'], spacer=channels['spacer'])
    if info is not None:
        info['height_margin'] = float(np.abs(my - channels['height']).min()) if len(my) else 1.0
    nx = np.minimum(np.maximum(px, 0.0), np.nextafter(bounds[0], 0.0))
    ny = np.minimum(np.maximum(my, 0.0), np.nextafter(bounds[1], 0.0))
    return nx, ny, pth, out


# ---------------------------------------------------------------------------
# the scenario: growing, dividing cells in channels
# ---------------------------------------------------------------------------

VOLUME_TO_FL = 1e-18 / 1e-3 * 1e18 * 1e-3     # as lens_amd.cells evaluates it
DENSITY = 1100.0


def capsule(width):
    radius = width / 2
    return (4 / 3) * math.pi * radius ** 3, math.pi * radius ** 2, 2 * radius


def derive(mass, width):
    """(volume fL, length) of DeriveGlobals, in vk_cell_step's order."""
    cap_volume, cap_area, two_r = capsule(width)
    raw = mass / DENSITY
    return raw * VOLUME_TO_FL, (raw - cap_volume) / cap_area + two_r


class Scenario:
    """The colony step of a mother machine with ``cells=`` (CellModel 'growth'), in the
    device's order: ``iterations`` contact iterations with the projection (the outflow
    flag sticks), growth from the step-start state with the division flag from the
    step-start volume, then the plan of division and removal and its gathers.  Keys are
    the column indices, as in a colony that was never sorted by bin."""

    def __init__(self, mm, *, jitter, iterations=4, seed=0, stiffness=0.5, max_length=4.0):
        self.bounds = tuple(float(b) for b in mm['bounds'])
        ch = mm['channels']
        self.channels = {'height': float(ch['channel_height']), 'space': float(ch['channel_space']),
                         'spacer': float(ch.get('spacer_thickness', 0.1))}
        self.width = float(mm['width'])
        self.factor = float(np.exp(mm['growth_rate'] * 1.0))
        self.division_volume = float(mm['division_volume'])
        self.kw = dict(stiffness=stiffness, max_length=max_length, width=self.width, jitter=jitter, seed=seed)
        self.iterations = iterations
        n = mm['location'].shape[1]
        self.x, self.y = mm['location'][0].astype(np.float64).copy(), mm['location'][1].astype(np.float64).copy()
        self.th = np.asarray(mm['angle'], dtype=np.float64).copy()
        self.mass = np.full(n, float(mm['mass']))
        self.volume, self.L = derive(self.mass, self.width)
        self.root = np.arange(n)
        self.root_channel = channel_of(self.x, self.bounds, self.channels['space'])
        self.counter = 0
        self.removed_per_channel = np.zeros(n_lines(self.bounds, self.channels['space']), dtype=np.int64)
        self.last_removed = 0
        self.newborn = np.zeros(n, dtype=bool)

    @property
    def n(self):
        return len(self.x)

    def contacts(self):
        """The contact launch: new x, y, theta in place; returns the outflow flags."""
        flagged = np.zeros(self.n, dtype=bool)
        for it in range(self.iterations):
            if self.n:
                self.x, self.y, self.th, out = iterate(self.x, self.y, self.th, self.L, np.arange(self.n),
                                                       self.bounds, self.counter + it, self.channels, **self.kw)
                flagged = out if it == 0 else (flagged | out)
        self.counter += self.iterations
        return flagged

    def grow_and_divide(self, flagged):
        divide = self.volume >= self.division_volume
        self.mass = self.mass * self.factor
        self.volume, self.L = derive(self.mass, self.width)
        src, kind, n_out = plan(divide, flagged, self.n)
        assert len(src) == n_out
        np.add.at(self.removed_per_channel, self.root_channel[self.root[flagged]], 1)
        self.last_removed = int(flagged.sum())
        daughter = kind >= 0
        half = lambda a: np.where(daughter, a[src] / 2.0, a[src])
        self.mass, self.volume, L = half(self.mass), half(self.volume), half(self.L)
        th = self.th[src]
        ratio = np.where(kind == 0, -0.25, 0.25)
        parent_length = L * 2.0
        self.x = np.where(daughter, self.x[src] + parent_length * ratio * np.cos(th), self.x[src])
        self.y = np.where(daughter, self.y[src] + parent_length * ratio * np.sin(th), self.y[src])
        self.th, self.L, self.root = th, L, self.root[src]
        self.newborn = daughter

    def step(self):
        self.grow_and_divide(self.contacts())

    def stale_above(self):
        """Whether an agent other than a daughter born in this step is above the channels."""
        return bool(((self.y > self.channels['height']) & ~self.newborn).any())

    def in_own_channels(self):
        """No agent in a channel other than its root's."""
        return bool((channel_of(self.x, self.bounds, self.channels['space']) == self.root_channel[self.root]).all())


def check_scenario(n_of, step_fn, in_own_channels, stale_above, removed_per_channel, steps, occupied):
    """The scenario's four assertions, checked after every step; returns the
    population after every step (the first entry is the start).

    'No agent above the channels at the end of a step' is asserted for every agent
    that took part in the step's contact launch: an agent the launch left above
    ``height`` is gone.  A daughter born in this step is placed L / 4 along its
    mother's axis after the launch and can start above ``height``; the next
    step's launch flags it, and that step's check covers it."""
    pop = [n_of()]
    for s in range(steps):
        step_fn()
        assert in_own_channels(), 'step %d: an agent is in a foreign channel' % s
        assert not stale_above(), 'step %d: an agent above the channels survived' % s
        pop.append(n_of())
    removed = removed_per_channel()
    assert all(removed[c] >= 1 for c in occupied), ('a channel never lost a cell', removed)
    d = np.diff(pop)
    assert (d > 0).any() and (d < 0).any(), 'the population is monotone'
    return pop
