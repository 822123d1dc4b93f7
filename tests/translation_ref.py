"""Restatement of the translation step (vk_translation_step) and of the ribosome divider
(vk_divide_ribosomes) as plain per-agent Python loops, for the tests.  It reads line by line
against the reference's Translation.next_update (vivarium/processes/translation.py:423-579)
and polymerize_step (vivarium/library/polymerize.py:205-259); the initiation is the direct
method include/vk_kinetics.h states above vk_translation_step, in vk_ssa_step's arithmetic:

    a_i       (affinity_i * float(unbound_i)) * float(ribosomes), 0 when either count is < 1
    total     a_0 + a_1 + ... in template order; cum_i the running sums
    draw e    Philox4x32-10, key seed ^ DOMAIN, counter (step, key, e, 0); u1 from words 0 and
              1, u2 from words 2 and 3; e counts every draw of the step, fired or not
    tau       -log(1.0 - u1) / total; t + tau > interval ends the sub-interval, and so does
              ribosomes < 1 (no draw)
    fire      the first q with cum_q > u2 * total

It contains its own scalar Philox pair; tests/test_translation_host.py checks it against
tests/ssa_ref.py.  ``model`` is a lens_amd.translation.TranslationModel, ``rows`` what its
bind() returns for the stochastic table.
"""

import math

import numpy as np

DOMAIN = 0x746c5f5f73746570            # VK_TL_DOMAIN
DIVIDE_DOMAIN = 0x746c5f5f64697669     # VK_TL_DIVIDE_DOMAIN
SLOTS_FULL, BAD_KEY, NONFINITE, OVERFLOW, MAX_EVENTS = 1, 2, 4, 8, 16
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
MARGIN = 1e-9
M32 = 0xFFFFFFFF


def philox_pair(seed, step, key, e):
    """(u1, u2): one Philox4x32-10 block, key (seed lo, seed hi), counter (step, key, e lo, e hi)."""
    seed = int(seed) & (2 ** 64 - 1)
    c0, c1, c2, c3 = int(step) & M32, int(key) & M32, int(e) & M32, (int(e) >> 32) & M32
    k0, k1 = seed & M32, seed >> 32
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
    u1 = (float(c0 >> 5) * 67108864.0 + float(c1 >> 6)) / 9007199254740992.0
    u2 = (float(c2 >> 5) * 67108864.0 + float(c3 >> 6)) / 9007199254740992.0
    return u1, u2


def plan(timestep, rate):
    """The sub-interval loop of translation.py:478-499, 533, alone."""
    out, time = [], 0
    while time < timestep:
        distance = 1 / rate
        interval = min(distance, timestep - time)
        out.append((interval, interval == distance))
        time += interval
    return out


def propensities(model, unbound, ribosomes):
    rib = 0.0 if ribosomes < 1 else float(ribosomes)
    out = []
    for i in range(model.n_templates):
        a = float(model.affinity[i])
        a = a * (0.0 if unbound[i] < 1 else float(unbound[i]))
        a = a * rib
        out.append(a)
    return out


def step_agent(model, rows, ribosomes, molecules, counts, key, timestep, seed, step_index, max_events=None,
               trace=None):
    """One step of one agent, in place: ``ribosomes`` a list of [template, position,
    occluding] in insertion order, ``molecules`` [monomers + 2] and ``counts`` [S] int
    arrays.  Returns (events, status bits, time margin, choice margin): the smallest
    |t + tau - interval| and |cum_i - u2 * total| / total she met (inf if she drew nothing).
    ``trace`` (a list) receives (sub-interval, 'elongate' | 'bind' | 'release', ...) records."""
    operon_species, prod_species, ribosome_species = rows
    T, M = model.n_templates, model.n_monomers
    max_events = model.max_events if max_events is None else int(max_events)
    key = int(key)
    if key < 0 or key > INT32_MAX:
        return 0, BAD_KEY, math.inf, math.inf
    kseed = (int(seed) ^ DOMAIN) & (2 ** 64 - 1)
    status = 0
    # gene - bound with bound = 0: no stored ribosome is 'bound' (translation.py:444-450)
    unbound = [int(counts[operon_species[i]]) for i in range(T)]
    free = int(counts[ribosome_species])
    limit = [int(molecules[m]) for m in range(M)]
    used = 0
    run, initiates = True, True
    events, e = 0, 0
    margin_t, margin_q = math.inf, math.inf
    for k, (interval, elongates) in enumerate(plan(timestep, model.elongation_rate)):
        # 1 the substrate, before elongation (translation.py:480-483)
        substrate_ribosomes, terminated = free, 0
        # 2 elongation (polymerize.py:221-257)
        if elongates:
            kept = []
            for ribosome in ribosomes:
                t, p = ribosome[0], ribosome[1]
                keep = True
                if run and t < T and p < model.length(t):
                    m = int(model.seq[model.seq_ptr[t] + p])
                    if limit[m] > 0:
                        products = prod_species[model.prod_ptr[t]:model.prod_ptr[t + 1]]
                        if p + 1 == model.length(t) and (
                                free == INT32_MAX or any(int(counts[s]) == INT32_MAX for s in products)):
                            status |= OVERFLOW
                            run = initiates = False
                        if run:
                            limit[m] -= 1
                            used += 1
                            ribosome[1] = p + 1
                            if ribosome[1] == model.length(t):
                                for s in products:
                                    counts[s] += 1
                                free += 1
                                terminated += 1
                                keep = False
                            if trace is not None:
                                trace.append((k, 'elongate', t, p + 1, not keep))
                if keep:
                    kept.append(ribosome)
            ribosomes[:] = kept
        # 3 initiation: the direct method over the sub-interval on the substrate
        now = 0.0
        active = initiates
        while active and substrate_ribosomes >= 1:
            a = propensities(model, unbound, substrate_ribosomes)
            total, cum = 0.0, []
            for a_i in a:
                total = total + a_i
                cum.append(total)
            if total == 0.0:
                break
            if not math.isfinite(total):
                status |= NONFINITE
                initiates = False
                break
            u1, u2 = philox_pair(kseed, step_index, key, e)
            e += 1
            tau = -math.log(1.0 - u1) / total
            margin_t = min(margin_t, abs(now + tau - interval))
            if now + tau > interval:
                break
            margin_q = min(margin_q, min(abs(c - u2 * total) for c in cum) / total)
            q = next((i for i in range(T) if cum[i] > u2 * total), T - 1)
            if len(ribosomes) >= model.max_ribosomes:
                status |= SLOTS_FULL
                initiates = False
                break
            now = now + tau
            unbound[q] -= 1
            substrate_ribosomes -= 1
            ribosomes.append([q, 0, True])
            events += 1
            if trace is not None:
                trace.append((k, 'bind', q))
            if events >= max_events:
                status |= MAX_EVENTS
                initiates = False
                break
        free = substrate_ribosomes + terminated
        # 4 release (translation.py:528-531): the reference always releases template 0
        if run:
            for ribosome in ribosomes:
                if ribosome[2] and ribosome[1] >= model.polymerase_occlusion:
                    ribosome[2] = False
                    r = ribosome[0] if model.release == 'template' else 0
                    unbound[r] += 1
                    if trace is not None:
                        trace.append((k, 'release', r, unbound[r]))
    counts[ribosome_species] = free
    for m in range(M):
        molecules[m] = limit[m]
    if used:
        atp, adp = int(molecules[M]) - 2 * used, int(molecules[M + 1]) + 2 * used
        if atp < INT32_MIN or adp > INT32_MAX:
            status |= OVERFLOW
        molecules[M], molecules[M + 1] = max(atp, INT32_MIN), min(adp, INT32_MAX)
    return events, status, margin_t, margin_q


def unpack_lists(slots, length, n):
    """Per agent a list of [template, position, occluding] from packed slots [cap, ld]."""
    out = []
    for a in range(n):
        words = np.asarray(slots[:int(length[a]), a]).astype(np.int64) & M32
        out.append([[int(w >> 1) & 63, int(w >> 7), bool(w & 1)] for w in words])
    return out


def pack_lists(lists, cap, ld):
    slots, length = np.zeros((cap, ld), dtype=np.int64), np.zeros(ld, dtype=np.int32)
    for a, ribosomes in enumerate(lists):
        length[a] = len(ribosomes)
        for j, (t, p, occluding) in enumerate(ribosomes):
            slots[j, a] = (p << 7) | (t << 1) | (1 if occluding else 0)
    return slots.astype(np.uint32).view(np.int32), length


def step(model, rows, lists, molecules, counts, keys, timestep, seed, step_index, status=None, max_events=None):
    """One step of agents [0, len(lists)) in place: ``lists`` per agent, ``molecules``
    [monomers + 2, >= n] and ``counts`` [S, >= n] int arrays.  Returns (events [n], status [n]
    with the bits OR-ed into ``status`` if given, time margin [n], choice margin [n])."""
    n = len(lists)
    status = np.zeros(n, dtype=np.int32) if status is None else status
    events, margin_t, margin_q = np.zeros(n, dtype=np.int32), np.full(n, np.inf), np.full(n, np.inf)
    for a in range(n):
        mol, x = molecules[:, a].astype(np.int64), counts[:, a].astype(np.int64)
        events[a], bits, margin_t[a], margin_q[a] = step_agent(
            model, rows, lists[a], mol, x, keys[a], timestep, seed, step_index, max_events)
        status[a] |= bits
        molecules[:, a], counts[:, a] = mol, x
    return events, status, margin_t, margin_q


def divide_ribosomes(lists, keys, src, kind, seed, step_index):
    """The lists over a plan: slot j takes agent src[j]; kind[j] < 0 is a survivor, else
    daughter kind[j], who takes every entry i of the mother whose coin falls on her:
    philox(seed ^ DIVIDE_DOMAIN; (step, mother key, 0, i)), first value, u < 0.5 -> 0."""
    kseed = (int(seed) ^ DIVIDE_DOMAIN) & (2 ** 64 - 1)
    out = []
    for j in range(len(src)):
        mother = lists[int(src[j])]
        if kind[j] < 0:
            out.append([list(r) for r in mother])
            continue
        mine = []
        for i, r in enumerate(mother):
            u, _ = philox_pair(kseed, step_index, keys[int(src[j])], i << 32)
            if (0 if u < 0.5 else 1) == int(kind[j]):
                mine.append(list(r))
        out.append(mine)
    return out


# -- the model and the cases of the tests -------------------------------------------------
SIZES = (1, 63, 64, 65, 257)          # one lane, a wave less one, a wave, a wave and one, several waves
CASE_SEED = 20261021                  # chosen on the CPU: no agent of any case below falls under MARGIN
SYMBOLS = {'a': 'Ala', 'b': 'Gly', 'c': 'Ser', 'd': 'Val'}
MONOMERS = ['Ala', 'Gly', 'Ser', 'Val']
SEQUENCES = {('o1', 'pX'): 'abc', ('o1', 'pY'): 'abcdabcddcba', ('o2', 'pZ'): 'dcbad'}
PRODUCTS = {('o1', 'pX'): ['pX'], ('o1', 'pY'): ['pY', 'pW'], ('o2', 'pZ'): ['pZ']}
SPECIES = ['o1', 'o2', 'pX', 'pY', 'pW', 'pZ', 'Ribosome', 'C1']


def template(key, length, products):
    """generate_template (polymerize.py:183-192) as data."""
    return {'id': key, 'position': 0, 'direction': 1, 'sites': [],
            'terminators': [{'position': length, 'strength': 1.0, 'products': list(products)}]}


def small_config(affinities=(0.3, 0.2, 0.5), rate=4.0, occlusion=2):
    """3 templates of 3, 12 and 5 residues on 2 operons, 4 monomers, one two-product terminator."""
    return dict(sequences=dict(SEQUENCES),
                templates={k: template(k, len(s), PRODUCTS[k]) for k, s in SEQUENCES.items()},
                transcript_affinities=dict(zip(SEQUENCES, affinities)), elongation_rate=rate,
                polymerase_occlusion=occlusion, symbol_to_monomer=dict(SYMBOLS), molecules=list(MONOMERS))


def small_stochastic(seed=0, rate=0.05):
    """The table of the small model: transcripts, proteins, the free ribosome and one complex
    pX + pZ -> C1."""
    from lens_amd.stochastic import StochasticModel
    return StochasticModel(SPECIES, {'complex': {'pX': -1, 'pZ': -1, 'C1': 1}}, {'complex': rate}, seed=seed)


def small_model(release='reference', max_ribosomes=8, seed=CASE_SEED, max_events=100000, **config):
    from lens_amd.translation import TranslationModel
    return TranslationModel(max_ribosomes=max_ribosomes, release=release, seed=seed, max_events=max_events,
                            **small_config(**config))


def step_case(n, release='reference', cap=8):
    """(model, stochastic model, lists, molecules [6, n + 7], counts [8, n + 7], keys [n + 7]) of
    the device tests.  Neighbouring lanes hold lists of length 0, 1, cap - 1 and cap; the pools
    are small, so ribosomes stall; columns >= n hold 7 and must stay."""
    rng = np.random.default_rng([CASE_SEED, n, cap])
    model, sm = small_model(release, cap), small_stochastic()
    ld = n + 7
    keys = rng.choice(2 ** 31, size=ld, replace=False).astype(np.int64)
    lists = []
    for a in range(n):
        ribosomes = []
        for _ in range((0, 1, cap - 1, cap)[a % 4]):
            t = int(rng.integers(0, 3))
            ribosomes.append([t, int(rng.integers(0, model.length(t))), bool(rng.integers(0, 2))])
        lists.append(ribosomes)
    molecules = rng.integers(0, 12, (6, ld)).astype(np.int32)
    molecules[4], molecules[5] = 1000, 0
    counts = rng.integers(0, 6, (8, ld)).astype(np.int32)
    molecules[:, n:], counts[:, n:] = 7, 7
    return model, sm, lists, molecules, counts, keys


def trajectory(model, rows, lists, molecules, counts, keys, timestep, steps, step0=0):
    """``steps`` steps of the case in place.  Returns per step (lists, molecules, counts, events,
    status) copies and the smallest time and choice margins any agent met."""
    import copy
    status = np.zeros(len(lists), dtype=np.int32)
    out, worst_t, worst_q = [], np.inf, np.inf
    for k in range(steps):
        events, status, margin_t, margin_q = step(model, rows, lists, molecules, counts, keys, timestep, model.seed,
                                                  step0 + k, status)
        worst_t, worst_q = min(worst_t, margin_t.min()), min(worst_q, margin_q.min())
        out.append((copy.deepcopy(lists), molecules.copy(), counts.copy(), events.copy(), status.copy()))
    return out, worst_t, worst_q
