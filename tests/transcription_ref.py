"""Restatement of the transcription step (vk_transcription_step) and of the RNAP divider as plain
per-agent Python loops, for the tests.  It reads line by line against the reference's
Transcription.next_update (vivarium/processes/transcription.py:370-553), polymerize_step,
BindingSite.state_when, Template.binding_state / strength_from / terminates_at
(vivarium/library/polymerize.py:87-160, 205-259); the engine's own parts are the ones
include/vk_kinetics.h names above vk_transcription_step:

    level     float(counts[factor]) / mmol_to_counts, at the start of the step
    a_p       (affinity_p * float(open_p)) * float(rnaps), 0 when either count is < 1
    total     a_0 + a_1 + ... in promoter order; cum_p the running sums
    draw e    Philox4x32-10, key seed ^ DOMAIN, counter (step, key, e, 0); u1 from words 0 and 1,
              u2 from words 2 and 3; e counts EVERY draw of the step in the order made: the
              read-through draws (u1 of their block) and the initiation draws, fired or not
    tau       -log(1.0 - u1) / total; t + tau > interval ends the sub-interval, and so does
              rnaps < 1 (no draw)
    fire      the first q with cum_q > u2 * total
    read-through   choice = u1 * strength_from(i); terminates iff choice <= strength[i]

``model`` is a lens_amd.transcription.TranscriptionModel, ``rows`` what its bind() returns for the
stochastic table.  The Philox pair is tests/translation_ref.py's (checked against tests/ssa_ref.py
by tests/test_transcription_host.py).
"""

import copy
import json
import math
import os

import numpy as np

from translation_ref import philox_pair, plan

DOMAIN = 0x74785f5f73746570            # VK_TX_DOMAIN
DIVIDE_DOMAIN = 0x74785f5f64697669     # VK_TX_DIVIDE_DOMAIN, mixed on the host into vk_divide_ribosomes' seed
TL_DIVIDE_DOMAIN = 0x746c5f5f64697669  # which vk_divide_ribosomes mixes in itself
SLOTS_FULL, BAD_KEY, NONFINITE, OVERFLOW, MAX_EVENTS = 1, 2, 4, 8, 16
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
MARGIN = 1e-9
M32 = 0xFFFFFFFF
NT = 4                                 # VK_TX_MAX_TERMINATORS: the stride of the per-terminator arrays
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def affinity_vector(model, thr_species, counts, m2c):
    """build_affinity_vector (transcription.py:240-248) over binding_state (polymerize.py:87-97,
    133-138).  Returns (affinity [P], the smallest |level - threshold| / threshold met)."""
    vector, margin, j = [], math.inf, 0
    for p in range(model.n_templates):
        state = []
        for factors, thresholds in zip(model.site_factors[p], model.site_thresholds[p]):
            found = None
            for factor, threshold in zip(factors, thresholds):
                level = float(np.float64(int(counts[thr_species[j]])) / np.float64(m2c))
                j += 1
                if threshold > 0:
                    margin = min(margin, abs(level - threshold) / threshold)
                if found is None and level >= threshold:
                    found = factor
            state.append(found)
        vector.append(model.affinity_of(p, state))
    return vector, margin


def propensities(model, affinity, blocked, rnaps):
    rn = 0.0 if rnaps < 1 else float(rnaps)
    out = []
    for p in range(model.n_templates):
        x = int(model.copy[p]) - blocked[p]
        a = float(affinity[p])
        a = a * (0.0 if x < 1 else float(x))
        a = a * rn
        out.append(a)
    return out


def step_agent(model, rows, rnaps, molecules, counts, m2c, key, timestep, seed, step_index, max_events=None,
               trace=None):
    """One step of one agent, in place: ``rnaps`` a list of [template, terminator, position,
    occluding] in insertion order, ``molecules`` [len(molecule_ids)] and ``counts`` [S] int arrays.
    Returns (events, status bits, margins): margins = the smallest |t + tau - interval|,
    |cum_i - u2 * total| / total, |choice - strength| / strength_from and |level - threshold| /
    threshold she met (inf where she met none).  ``trace`` (a list) receives (sub-interval,
    'elongate' | 'bind' | 'unocclude' | 'readthrough', ...) records."""
    prod_ptr, prod_species, thr_species, rnap_species = rows
    P, M = model.n_templates, model.n_monomers
    max_events = model.max_events if max_events is None else int(max_events)
    key = int(key)
    if key < 0 or key > INT32_MAX:
        return 0, BAD_KEY, [math.inf] * 4
    kseed = (int(seed) ^ DOMAIN) & (2 ** 64 - 1)
    status = 0
    # the affinity vector, once, before the loop (transcription.py:425)
    affinity, margin_l = affinity_vector(model, thr_species, counts, m2c)
    # blocked promoters: the stored RNAPs that are occluding (transcription.py:388-396)
    blocked = [0] * P
    for rnap in rnaps:
        if rnap[3] and rnap[0] < P:
            blocked[rnap[0]] += 1
    free = int(counts[rnap_species])
    limit = [int(molecules[m]) for m in range(M)]
    used = [0] * M
    run, initiates = True, True
    events, e = 0, 0
    margin_t, margin_q, margin_c = math.inf, math.inf, math.inf
    for k, (interval, elongates) in enumerate(plan(timestep, model.elongation_rate)):
        # 1 the substrate, before elongation (transcription.py:429-432)
        substrate_rnaps, terminated = free, 0
        # 2 elongation (polymerize.py:221-257): occluding or polymerizing, in list order
        if elongates:
            kept = []
            for rnap in rnaps:
                t, i, p = rnap[0], rnap[1], rnap[2]
                keep = True
                if run and t < P and p < model.length(t):
                    m = int(model.seq[model.seq_ptr[t] + p])
                    if limit[m] > 0:
                        ix = NT * t + i
                        at = p + 1 == int(model.term_pos[ix])
                        products = prod_species[prod_ptr[ix]:prod_ptr[ix + 1]]
                        if at and (free == INT32_MAX or any(int(counts[s]) == INT32_MAX for s in products)):
                            status |= OVERFLOW
                            run = initiates = False
                        if run:
                            limit[m] -= 1
                            used[m] += 1
                            rnap[2] = p + 1
                            if at:
                                # terminates_at (polymerize.py:155-160)
                                if i + 1 < int(model.n_term[t]):
                                    u1, _ = philox_pair(kseed, step_index, key, e)
                                    e += 1
                                    choice = u1 * float(model.term_from[ix])
                                    ends = choice <= float(model.term_strength[ix])
                                    margin_c = min(margin_c, abs(choice - float(model.term_strength[ix])) /
                                                   float(model.term_from[ix]))
                                    if trace is not None:
                                        trace.append((k, 'readthrough', t, i, ends))
                                else:
                                    ends = True
                                if ends:
                                    for s in products:
                                        counts[s] += 1
                                    free += 1
                                    terminated += 1
                                    keep = False
                                else:
                                    rnap[1] = i + 1
                            if trace is not None:
                                trace.append((k, 'elongate', t, p + 1, not keep))
                if keep:
                    kept.append(rnap)
            rnaps[:] = kept
        # 3 initiation: the direct method over the sub-interval on the substrate
        now = 0.0
        active = initiates
        while active and substrate_rnaps >= 1:
            a = propensities(model, affinity, blocked, substrate_rnaps)
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
            q = next((i for i in range(P) if cum[i] > u2 * total), P - 1)
            if len(rnaps) >= model.max_rnaps:
                status |= SLOTS_FULL
                initiates = False
                break
            now = now + tau
            blocked[q] += 1
            substrate_rnaps -= 1
            rnaps.append([q, 0, 0, True])                # bind_rnap, start_polymerizing (:479-480)
            events += 1
            if trace is not None:
                trace.append((k, 'bind', q))
            if events >= max_events:
                status |= MAX_EVENTS
                initiates = False
                break
        free = substrate_rnaps + terminated
        # 4 unocclusion (transcription.py:487-494): her own template reopens
        if run:
            for rnap in rnaps:
                if rnap[3] and rnap[2] >= model.polymerase_occlusion:
                    rnap[3] = False
                    if rnap[0] < P:
                        blocked[rnap[0]] -= 1
                    if trace is not None:
                        trace.append((k, 'unocclude', rnap[0]))
    counts[rnap_species] = free
    # the books (transcription.py:507-516): -used per monomer, ATP's entry overwritten, then the cost
    update = {m: -used[m] for m in range(M)}
    update[model.atp_row] = 0
    update[model.adp_row] = 0
    for count in used:
        update[model.atp_row] -= count
        update[model.adp_row] += count
    if sum(used):
        for r, delta in update.items():
            molecules[r] = int(molecules[r]) + delta
        if molecules[model.atp_row] < INT32_MIN or molecules[model.adp_row] > INT32_MAX:
            status |= OVERFLOW
        molecules[model.atp_row] = max(int(molecules[model.atp_row]), INT32_MIN)
        molecules[model.adp_row] = min(int(molecules[model.adp_row]), INT32_MAX)
    return events, status, [margin_t, margin_q, margin_c, margin_l]


def unpack_lists(slots, length, n):
    """Per agent a list of [template, terminator, position, occluding] from packed slots [cap, ld]."""
    out = []
    for a in range(n):
        words = np.asarray(slots[:int(length[a]), a]).astype(np.int64) & M32
        out.append([[int(w >> 1) & 63, int(w >> 7) & 3, int(w >> 9), bool(w & 1)] for w in words])
    return out


def pack_lists(lists, cap, ld):
    slots, length = np.zeros((cap, ld), dtype=np.int64), np.zeros(ld, dtype=np.int32)
    for a, rnaps in enumerate(lists):
        length[a] = len(rnaps)
        for j, (t, i, p, occluding) in enumerate(rnaps):
            slots[j, a] = (p << 9) | (i << 7) | (t << 1) | (1 if occluding else 0)
    return slots.astype(np.uint32).view(np.int32), length


def step(model, rows, lists, molecules, counts, m2c, keys, timestep, seed, step_index, status=None, max_events=None):
    """One step of agents [0, len(lists)) in place.  Returns (events [n], status [n] with the bits
    OR-ed into ``status`` if given, margins [n, 4])."""
    n = len(lists)
    status = np.zeros(n, dtype=np.int32) if status is None else status
    events, margins = np.zeros(n, dtype=np.int32), np.full((n, 4), np.inf)
    for a in range(n):
        mol, x = molecules[:, a].astype(np.int64), counts[:, a].astype(np.int64)
        events[a], bits, margins[a] = step_agent(model, rows, lists[a], mol, x, m2c[a], keys[a], timestep, seed,
                                                 step_index, max_events)
        status[a] |= bits
        molecules[:, a], counts[:, a] = mol, x
    return events, status, margins


def divide_rnaps(lists, keys, src, kind, seed, step_index):
    """The lists over a plan, as vk_divide_ribosomes deals them with the seed the host mixes:
    philox((seed ^ DIVIDE_DOMAIN) ^ TL_DIVIDE_DOMAIN; (step, mother key, 0, i)), u < 0.5 -> 0."""
    kseed = (int(seed) ^ DIVIDE_DOMAIN ^ TL_DIVIDE_DOMAIN) & (2 ** 64 - 1)
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
SPECIES = ['oA', 'oAZ', 'oB', 'oBY', 'tfA', 'tfB', 'RNA Polymerase', 'X']
TIMESTEP = 0.55                       # five elongating sub-intervals of 0.1 s and a partial one


def toy_data():
    return json.load(open(os.path.join(GOLDEN, 'toy_chromosome.json')))


def flagella_data():
    return json.load(open(os.path.join(GOLDEN, 'flagella_transcription.json')))


def toy_stochastic(seed=0, rate=0.05):
    """The table of the toy model: the four operons, the two factors, the free RNAP and one species
    more; oA decays."""
    from lens_amd.stochastic import StochasticModel
    return StochasticModel(SPECIES, {'decay': {'oA': -1, 'X': 1}}, {'decay': rate}, seed=seed)


def toy_model(max_rnaps=8, seed=CASE_SEED, affinity=None, **model):
    """The toy chromosome of the fixture; ``affinity`` replaces every promoter affinity."""
    from lens_amd import configs
    data = toy_data()
    if affinity is not None:
        data['promoter_affinities'] = [[k, affinity] for k, _ in data['promoter_affinities']]
    return configs.toy_transcription(data, max_rnaps=max_rnaps, seed=seed, **model)


def random_rnap(model, rng):
    t = int(rng.integers(0, model.n_templates))
    i = int(rng.integers(0, int(model.n_term[t])))
    lo = model.term_pos_rel[t][i - 1] if i else 0
    return [t, i, int(rng.integers(lo, model.term_pos_rel[t][i])), bool(rng.integers(0, 2))]


def step_case(n, cap=8, free=True, seed=CASE_SEED, **model):
    """(model, stochastic model, lists, molecules [5, n + 7], counts [8, n + 7], m2c [n + 7], keys
    [n + 7]) of the device tests.  Neighbouring lanes hold lists of length 0, 1, cap - 1 and cap;
    the pools are small, so RNAPs stall; mmol_to_counts differs from agent to agent and the
    factor counts sit on both sides of both thresholds; columns >= n hold 7 and must stay."""
    rng = np.random.default_rng([seed, n, cap])
    model, sm = toy_model(cap, seed=seed, **model), toy_stochastic()
    ld = n + 7
    keys = rng.choice(2 ** 31, size=ld, replace=False).astype(np.int64)
    lists = [[random_rnap(model, rng) for _ in range((0, 1, cap - 1, cap)[a % 4])] for a in range(n)]
    molecules = rng.integers(0, 14, (5, ld)).astype(np.int32)
    molecules[4] = 0
    counts = rng.integers(0, 6, (8, ld)).astype(np.int32)
    m2c = rng.uniform(5.0, 40.0, ld)
    # levels of 0.1 .. 0.9 mM around the thresholds 0.3 and 0.5, never on one
    for row, f in ((4, 0), (5, 1)):
        level = rng.choice([0.11, 0.29, 0.31, 0.49, 0.52, 0.9], size=ld)
        counts[row] = np.maximum(np.rint(level * m2c), 0).astype(np.int32)
    counts[6] = rng.integers(0, 5, ld) if free else 0
    molecules[:, n:], counts[:, n:] = 7, 7
    return model, sm, lists, molecules, counts, m2c, keys


def trajectory(model, rows, lists, molecules, counts, m2c, keys, timestep, steps, step0=0):
    """``steps`` steps of the case in place.  Returns per step (lists, molecules, counts, events,
    status) copies and the smallest margins any agent met: [time, choice of promoter,
    read-through, level]."""
    status = np.zeros(len(lists), dtype=np.int32)
    out, worst = [], np.full(4, np.inf)
    for k in range(steps):
        events, status, margins = step(model, rows, lists, molecules, counts, m2c, keys, timestep, model.seed,
                                       step0 + k, status)
        if len(lists):
            worst = np.minimum(worst, margins.min(axis=0))
        out.append((copy.deepcopy(lists), molecules.copy(), counts.copy(), events.copy(), status.copy()))
    return out, worst
