"""Restatement of the RNA degradation step (vk_rna_degradation_step) as plain per-agent Python
loops over NumPy float64 scalars, for the tests.  It reads line by line against the reference's
RnaDegradation.next_update (vivarium/processes/degradation.py:136-182):

    :146-153  for protein, kcat / for transcript, km: delta[transcript] += kinetics(E, S, kcat, km)
              with E = proteins[protein] / mmol_to_counts, S = transcripts[transcript] /
              mmol_to_counts and kinetics = kcat * E * S / (S + km) -- here regrouped per
              transcript, which keeps each transcript's order of summation (the enzymes in
              catalytic_rates order);
    :155-158  level * mmol_to_counts * timestep + partial_transcripts[transcript];
    :160-166  -int(level) and level - int(level);
    :172-178  delta_molecules[nucleotides[base]] -= count, ATP -= count, ADP += count with a
              NEGATIVE count: the monomers and ATP rise, ADP falls.

The engine's own parts are the ones include/vk_kinetics.h names above vk_rna_degradation_step: km
in mM by lens_amd.degradation.KM_TO_MM, the clamp d <= counts[t], the saturation of d to int32,
and the refusal (nothing written) of an agent whose mmol_to_counts or totals are not finite or
whose pools would leave int32.

``model`` is a lens_amd.degradation.DegradationModel, ``rows`` what its bind() returns.
"""

import json
import math
import os

import numpy as np

NONFINITE, OVERFLOW = 1, 2
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIZES = (1, 63, 64, 65, 257)          # one lane, a wave less one, a wave, a wave and one, more than a block
SENTINEL = 7                          # what columns n..ld-1 hold
f64 = np.float64


def step_agent(model, rows, counts, partial, molecules, m2c, timestep):
    """One step of one agent, in place: ``counts`` [n_rows] and ``molecules`` [len(molecule_ids)]
    int arrays, ``partial`` [n_transcripts] float64.  Returns (degraded, status bits); with a bit
    set nothing was written."""
    transcript_row, enzyme_row = rows
    m, T = f64(m2c), f64(timestep)
    bad = not (math.isfinite(m) and m > 0)
    d_all, carry = [], []
    with np.errstate(all='ignore'):
        for t in range(model.n_transcripts):
            level = f64(0.0)
            for j in range(int(model.pair_ptr[t]), int(model.pair_ptr[t + 1])):
                e = int(enzyme_row[model.pair_enzyme[j]])
                E = f64(int(counts[e])) / m
                S = f64(int(counts[transcript_row[t]])) / m
                level = level + ((f64(model.pair_kcat[j]) * E) * S) / (S + f64(model.pair_km[j]))
            total = (level * m) * T + f64(partial[t])
            if not math.isfinite(total):
                bad = True
                d_all.append(0)
                carry.append(f64(0.0))
                continue
            whole = np.trunc(total)
            carry.append(total - whole)
            d = min(max(int(whole), INT32_MIN), INT32_MAX)
            d_all.append(min(d, int(counts[transcript_row[t]])))         # the engine's own clamp
    if bad:
        return 0, NONFINITE
    M = model.n_monomers
    after = [int(x) for x in molecules]
    for t, d in enumerate(d_all):
        for i in range(M):
            after[i] += d * int(model.composition[t, i])
        after[model.atp_row] += d * int(model.length[t])
        after[model.adp_row] -= d * int(model.length[t])
    if any(x > INT32_MAX or x < INT32_MIN for x in after):
        return 0, OVERFLOW
    for t, d in enumerate(d_all):
        counts[transcript_row[t]] -= d
        partial[t] = carry[t]
    molecules[:] = after
    return min(max(sum(d_all), INT32_MIN), INT32_MAX), 0


def step(model, rows, counts, partial, molecules, m2c, timestep, n=None, status=None):
    """One step in place for agents [0, n) of counts [n_rows, ld], partial [T, ld], molecules [R, ld]
    with m2c [ld].  Returns (degraded [n] int32, status [n] int32 with the bits OR-ed into
    ``status`` if given)."""
    n = counts.shape[1] if n is None else n
    status = np.zeros(n, dtype=np.int32) if status is None else status
    degraded = np.zeros(n, dtype=np.int32)
    for a in range(n):
        x, p, mol = counts[:, a].copy(), partial[:, a].copy(), molecules[:, a].copy()
        degraded[a], bits = step_agent(model, rows, x, p, mol, m2c[a], timestep)
        status[a] |= bits
        counts[:, a], partial[:, a], molecules[:, a] = x, p, mol
    return degraded, status


# -- the models and the cases of the tests --------------------------------------------------
def toy_data():
    return json.load(open(os.path.join(GOLDEN, 'toy_degradation.json')))


def flagella_data():
    return json.load(open(os.path.join(GOLDEN, 'flagella_degradation.json')))


def toy_model(**model):
    from lens_amd import configs
    return configs.toy_degradation(toy_data(), **model)


class Pools:
    """What DegradationModel.bind asks of a TranscriptionModel, for cases without a chromosome."""

    def __init__(self, molecule_ids):
        self.molecule_ids = list(molecule_ids)


def bind(model, rows_of_table):
    """(transcript_row, enzyme_row) of ``model`` in a table whose rows are ``rows_of_table``."""
    return (np.asarray([rows_of_table.index(s) for s in model.transcript_names()], dtype=np.int32),
            np.asarray([rows_of_table.index(s) for s in model.enzyme_order], dtype=np.int32))


def case(model, table_rows, n, seed, enzymes=(0, 41), transcripts=(0, 30), m2c=(5.0, 40.0), pools=(0, 1000)):
    """(counts [n_rows, ld], partial [T, ld], molecules [R, ld], m2c [ld]) with ld = n + 7: counts of
    the enzymes, the transcripts and every other row drawn per agent, mmol_to_counts differing
    from agent to agent, columns >= n holding SENTINEL."""
    rng = np.random.default_rng([seed, n])
    ld = n + 7
    trow, erow = bind(model, table_rows)
    counts = rng.integers(0, 50, (len(table_rows), ld)).astype(np.int32)
    counts[trow] = rng.integers(*transcripts, (len(trow), ld))
    counts[erow] = rng.integers(*enzymes, (len(erow), ld))
    partial = np.zeros((model.n_transcripts, ld))
    molecules = rng.integers(*pools, (len(model.molecule_ids), ld)).astype(np.int32)
    m = rng.uniform(*m2c, ld)
    counts[:, n:], partial[:, n:], molecules[:, n:], m[n:] = SENTINEL, SENTINEL, SENTINEL, SENTINEL
    return counts, partial, molecules, m
