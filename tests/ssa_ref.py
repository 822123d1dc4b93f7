"""NumPy restatement of the batched Gillespie step (vk_ssa_step, vk_ssa_propensities),
of divide_split on int counts (vk_divide_counts) and of the flagella target
(vk_ssa_flagella_target), for the tests.  Vectorised over agents; the arithmetic is the
one include/vk_kinetics.h states above vk_ssa_step, operation for operation:

    C(n, k)   0 if n < k, else c = 1.0; for i < k: c = c * float64(n - i); c = c * inv[i]
    a_r       rate_r, then a = a * C(x_s, k) per reactant in ascending species order
    total     a_0 + a_1 + ... in reaction order; cum_r the running sums
    draw e    Philox4x32-10, key seed ^ DOMAIN, counter (step, key, e, 0); u1 from words
              0 and 1, u2 from words 2 and 3
    tau       -log(1.0 - u1) / total; stop if t + tau > T
    fire      the first q with cum_q > u2 * total

It contains its own Philox pair; tests/test_ssa_host.py checks its first value against
oracle.colony.philox_uniform.  ``model`` is a lens_amd.stochastic.StochasticModel (only
its packed host arrays are read).
"""

import numpy as np

DOMAIN = 0x7373615f73746570            # VK_SSA_DOMAIN
DIVIDE_DOMAIN = 0x7373615f64697669     # VK_SSA_DIVIDE_DOMAIN
MAX_EVENTS, NONFINITE, OVERFLOW, BAD_KEY = 1, 2, 4, 8
INT32_MAX = 2 ** 31 - 1
M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox_pair(seed, step, key, e):
    """(u1, u2) float64 arrays: one Philox4x32-10 block per element of ``key`` / ``e``
    (broadcast), key (seed lo, seed hi), counter (step, key, e lo, e hi)."""
    key, e = np.broadcast_arrays(np.asarray(key, dtype=np.int64), np.asarray(e, dtype=np.int64))
    seed = int(seed) & (2 ** 64 - 1)
    c0 = np.full(key.shape, int(step) & 0xFFFFFFFF, dtype=np.uint64)
    c1 = key.astype(np.uint64) & M32
    c2 = e.astype(np.uint64) & M32
    c3 = (e.astype(np.uint64) >> _S32) & M32
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, \
                         ((p0 >> _S32) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
    five, six = np.uint64(5), np.uint64(6)
    u1 = ((c0 >> five).astype(np.float64) * 67108864.0 + (c1 >> six).astype(np.float64)) / 9007199254740992.0
    u2 = ((c2 >> five).astype(np.float64) * 67108864.0 + (c3 >> six).astype(np.float64)) / 9007199254740992.0
    return u1, u2


def choose(n, k, inv=None):
    """C(n, k) of an int array n, as the kernel multiplies it out (float64)."""
    n = np.asarray(n, dtype=np.int64)
    if inv is None:
        inv = 1.0 / np.arange(1, 256, dtype=np.float64)
    c = np.ones(n.shape, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for i in range(int(k)):
            c = c * (n - i).astype(np.float64)
            c = c * inv[i]
    return np.where(n < k, 0.0, c)


def propensities(model, x):
    """a [R, n] float64 of counts x [S, n]."""
    x = np.asarray(x)
    a = np.empty((model.n_reactions, x.shape[1]), dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for r in range(model.n_reactions):
            v = np.full(x.shape[1], model.rates[r], dtype=np.float64)
            for j in range(model.react_ptr[r], model.react_ptr[r + 1]):
                v = v * choose(x[model.react_species[j]], model.react_order[j], model.inv)
            a[r] = v
    return a


def step(model, x, keys, duration, seed, step_index, max_events=None, status=None):
    """One step in place on x [S, n] (an int array) for the agents with ``keys`` [n].
    Returns (events [n] int32, status [n] int32 with the bits OR-ed into ``status`` if
    given, margin [n]): margin is the smallest |t + tau - T| / T the agent met in this
    step (inf if she drew nothing)."""
    S, n = x.shape
    R = model.n_reactions
    keys = np.asarray(keys, dtype=np.int64)
    max_events = model.max_events if max_events is None else int(max_events)
    T = float(duration)
    status = np.zeros(n, dtype=np.int32) if status is None else status
    bad = (keys < 0) | (keys > INT32_MAX)
    status[bad] |= BAD_KEY
    active = ~bad
    t = np.zeros(n)
    events = np.zeros(n, dtype=np.int64)
    margin = np.full(n, np.inf)
    matrix = model.matrix                                   # [R, S] int64
    kseed = (int(seed) ^ DOMAIN) & (2 ** 64 - 1)
    while active.any():
        idx = np.nonzero(active)[0]
        a = propensities(model, x[:, idx])
        cum = np.empty_like(a)
        total = np.zeros(len(idx))
        with np.errstate(over='ignore', invalid='ignore'):
            for r in range(R):
                total = total + a[r]
                cum[r] = total
        zero = total == 0.0
        nonfinite = ~np.isfinite(total)
        status[idx[nonfinite]] |= NONFINITE
        active[idx[zero | nonfinite]] = False
        go = ~(zero | nonfinite)
        idx, cum, total = idx[go], cum[:, go], total[go]
        if not len(idx):
            break
        u1, u2 = philox_pair(kseed, step_index, keys[idx], events[idx])
        tau = -np.log(1.0 - u1) / total
        if T > 0:
            margin[idx] = np.minimum(margin[idx], np.abs(t[idx] + tau - T) / T)
        stop = t[idx] + tau > T
        active[idx[stop]] = False
        go = ~stop
        idx, cum, total, tau, u2 = idx[go], cum[:, go], total[go], tau[go], u2[go]
        if not len(idx):
            continue
        t[idx] = t[idx] + tau
        hit = cum > (u2 * total)[None, :]
        q = np.where(hit.any(axis=0), hit.argmax(axis=0), R - 1)
        new = x[:, idx].astype(np.int64) + matrix[q].T
        over = (new > INT32_MAX).any(axis=0)
        status[idx[over]] |= OVERFLOW
        active[idx[over]] = False
        ok = idx[~over]
        x[:, ok] = new[:, ~over].astype(x.dtype)
        events[ok] += 1
        full = ok[events[ok] >= max_events]
        status[full] |= MAX_EVENTS
        active[full] = False
    return events.astype(np.int32), status, margin


def split_int(x, u):
    """divide_split on ints (core/registry.py:205-227): (daughter 0, daughter 1); half =
    int(x / 2), the odd one to daughter 0 exactly when u < 0.5."""
    x = np.asarray(x, dtype=np.int64)
    half = np.trunc(x / 2).astype(np.int64)
    rest = x - 2 * half
    first = np.asarray(u) < 0.5
    return half + np.where(first, rest, 0), half + np.where(first, 0, rest)


def divide_counts(x, keys, src, kind, n_keep, seed, step_index, key_base):
    """(x' [S, n_out], keys' [n_out]) over a plan: slot j takes agent src[j]; kind[j] < 0
    is a survivor, else daughter kind[j] of that mother.  One coin per (mother, species):
    philox(seed ^ DIVIDE_DOMAIN; (step, mother key, species, 0)), first value."""
    x, keys = np.asarray(x), np.asarray(keys, dtype=np.int64)
    src, kind = np.asarray(src, dtype=np.int64), np.asarray(kind, dtype=np.int64)
    S, n_out = x.shape[0], len(src)
    out = x[:, src].astype(np.int64)
    new_keys = keys[src].copy()
    d = np.nonzero(kind >= 0)[0]
    new_keys[d] = key_base + (d - n_keep)
    kseed = (int(seed) ^ DIVIDE_DOMAIN) & (2 ** 64 - 1)
    for s in range(S):
        u, _ = philox_pair(kseed, step_index, keys[src[d]], np.full(len(d), s))
        d0, d1 = split_int(x[s, src[d]], u)
        out[s, d] = np.where(kind[d] == 0, d0, d1)
    return out.astype(x.dtype), new_keys


def flagella_target(row):
    """(target int32, flag): clamp(count, 0, 32); flag: some count lay outside 0..32."""
    row = np.asarray(row, dtype=np.int64)
    return np.clip(row, 0, 32).astype(np.int32), bool(((row < 0) | (row > 32)).any())


def trajectory(model, x0, keys, n, duration, steps, max_events=None, step0=0):
    """``steps`` steps of agents [0, n) of x0 [S, ld] (columns >= n stay).  Returns a list of
    (x [S, ld], events [n], status [n]) per step and ``out`` [n] bool: the agents whose time
    margin fell below MARGIN in this or an earlier step (their later draws may differ too)."""
    x = np.array(x0, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    out = np.zeros(n, dtype=bool)
    result = []
    for k in range(steps):
        part = x[:, :n].copy()
        events, status, margin = step(model, part, keys[:n], duration, model.seed, step0 + k, max_events, status)
        x[:, :n] = part
        out |= margin < MARGIN
        result.append((x.copy(), events.copy(), status.copy()))
    return result, out


MARGIN = 1e-9
SIZES = (1, 63, 64, 65, 257)          # one lane, a wave less one, a wave, a wave and one, several waves
CASE_SEED = 20261020                  # chosen on the CPU: no agent of any case below falls under MARGIN


def step_case(net, n):
    """(model, x0 [S, n + 7] int32, keys [n + 7] int64, duration, max_events) of the device
    tests: the fixture network with counts in 0..300, the birth-death network from 0, a
    random network at the limits (stopped after 20 events: its propensities are huge).
    Keys are distinct and spread over [0, 2**31); columns >= n hold 7 and must stay."""
    rng = np.random.default_rng([CASE_SEED, n, ('fixture', 'birth_death', 'limits').index(net)])
    ld = n + 7
    keys = rng.choice(2 ** 31, size=ld, replace=False).astype(np.int64)
    if net == 'fixture':
        model, max_events = fixture_model(seed=CASE_SEED), None
        x0 = rng.integers(0, 301, (model.n_species, ld))
    elif net == 'birth_death':
        model, max_events = birth_death_model(seed=CASE_SEED + 1), None
        x0 = np.zeros((1, ld))
    else:
        model, max_events = limits_model(seed=CASE_SEED + 2), 20
        x0 = rng.integers(0, 301, (model.n_species, ld))
    x0 = x0.astype(np.int32)
    x0[:, n:] = 7
    return model, x0, keys, 1.0, max_events


# -- the networks of the tests ------------------------------------------------------------
def load_fixture():
    """tests/golden/flagella_complexation.json: the reference's complexation network."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flagella_complexation.json')) as f:
        return json.load(f)


def fixture_model(initial_monomers=0, seed=0, max_events=100000):
    from lens_amd.stochastic import StochasticModel
    fx = load_fixture()
    species = fx['monomer_ids'] + fx['complex_ids']
    return StochasticModel(species, fx['stoichiometry'], fx['rates'],
                           initial={m: initial_monomers for m in fx['monomer_ids']}, seed=seed, max_events=max_events)


def birth_death_model(seed=0, birth=50.0, death=0.5):
    from lens_amd.stochastic import StochasticModel
    return StochasticModel(['X'], {'birth': {'X': 1}, 'death': {'X': -1}}, {'birth': birth, 'death': death}, seed=seed)


def birth_model(seed=0, birth=50.0):
    from lens_amd.stochastic import StochasticModel
    return StochasticModel(['X'], {'birth': {'X': 1}}, {'birth': birth}, seed=seed)


def limits_model(seed=0):
    """A random network at the limits: 64 species, 32 reactions, orders up to 255."""
    from lens_amd.stochastic import StochasticModel
    rng = np.random.default_rng(12345)
    species = ['s%d' % i for i in range(64)]
    stoich = {}
    for r in range(32):
        members = rng.choice(64, size=int(rng.integers(1, 6)), replace=False)
        row = {}
        for i, s in enumerate(members):
            if i == 0 and r % 4 == 0:
                row[species[s]] = -int(rng.choice([255, 200, 120]))
            elif rng.random() < 0.6:
                row[species[s]] = -int(rng.integers(1, 5))
            else:
                row[species[s]] = int(rng.integers(1, 4))
        stoich['r%d' % r] = row
    stoich['r31'] = {species[63]: 2}                       # a reaction without reactants
    rates = {rid: float(10.0 ** rng.uniform(-6, 1)) for rid in stoich}
    return StochasticModel(species, stoich, rates, seed=seed)
