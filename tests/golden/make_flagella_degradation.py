"""Generate tests/golden/flagella_degradation.json and tests/golden/toy_degradation.json (run once
where the reference tree is).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flagella_degradation.py REFERENCE_ROOT

The degradation config of the reference's flagella agent
(vivarium/compartments/flagella_expression.py:119-128) needs FlagellaChromosome, which does not
import without ``pint``, so this script reads the data out of the source files with ``ast``
(nothing of the reference is executed):

* ``catalytic_rates``: ``{'endoRNAse': 0.02}``;
* ``michaelis_constants``: ``{'transcripts': {'endoRNAse': {operon: 1e-23}}}`` over the operons
  of ``chromosome_config['genes']`` in the reference's order, each km the plain magnitude the
  reference multiplies by ``units.mole / units.fL`` (vivarium/processes/degradation.py:148);
* ``initial_state``: ``get_flagella_initial_state`` (flagella_expression.py:318-349): the
  ``molecules`` (5 000 000 of every nucleotide, 1 000 000 of every amino acid), the
  ``transcripts`` (0 of every operon) and the ``proteins`` with the names UNBOUND_RIBOSOME_KEY and
  UNBOUND_RNAP_KEY resolved from the process modules.

The sequences are NOT in the file: the reference takes them from
``Chromosome.product_sequences()`` over a genome its tree does not hold;
lens_amd.configs.flagella_degradation takes them from the TranscriptionModel.

``toy_degradation.json`` is ``TOY_CONFIG`` (vivarium/processes/degradation.py:30-50) with the
initial state of ``test_rna_degradation`` (:185-207).

Nothing here is imported at test time; tests read only the written files.
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _parse(root, *path):
    return ast.parse(open(os.path.join(root, 'vivarium', *path)).read())


def _assigned(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id == name:
            return node.value
    raise KeyError(name)


def _entry(node, key):
    for k, v in zip(node.keys, node.values):
        if isinstance(k, ast.Constant) and k.value == key:
            return v
    raise KeyError(key)


def _function(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


class _Names(ast.NodeTransformer):
    """A module-level constant's name -> its value."""

    def __init__(self, values):
        self.values = values

    def visit_Name(self, node):
        return ast.Constant(self.values[node.id]) if node.id in self.values else node


def _literal(node, names=None):
    return ast.literal_eval(ast.fix_missing_locations(_Names(names or {}).visit(node)))


def write(name, out):
    path = os.path.join(HERE, name)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    return path


def main(root):
    chromosome = _parse(root, 'data', 'chromosomes', 'flagella_chromosome.py')
    genes = None
    for d in (n for n in ast.walk(chromosome) if isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and k.value == 'genes' and isinstance(v, ast.Dict):
                genes = ast.literal_eval(v)
    operons = list(genes.keys())
    expr = _parse(root, 'compartments', 'flagella_expression.py')
    config = None
    for d in (n for n in ast.walk(expr) if isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and k.value == 'degradation' and isinstance(v, ast.Dict) and any(
                    isinstance(kk, ast.Constant) and kk.value == 'catalytic_rates' for kk in v.keys):
                config = v
    rates = ast.literal_eval(_entry(config, 'catalytic_rates'))
    kms = {}
    transcripts = _entry(_entry(config, 'michaelis_constants'), 'transcripts')
    for enzyme, comp in zip(transcripts.keys, transcripts.values):
        # {transcript: 1e-23 for transcript in chromosome_config['genes'].keys()}
        assert isinstance(comp, ast.DictComp) and isinstance(comp.key, ast.Name)
        kms[enzyme.value] = {operon: ast.literal_eval(comp.value) for operon in operons}
    names = {'UNBOUND_RIBOSOME_KEY': ast.literal_eval(_assigned(_parse(root, 'processes', 'translation.py'),
                                                                'UNBOUND_RIBOSOME_KEY')),
             'UNBOUND_RNAP_KEY': ast.literal_eval(_assigned(_parse(root, 'processes', 'transcription.py'),
                                                            'UNBOUND_RNAP_KEY'))}
    nucleotides = ast.literal_eval(_assigned(_parse(root, 'data', 'nucleotides.py'), 'nucleotides'))
    # amino_acids = {record['symbol']: record['name'] for record in amino_acid_records}
    amino_acids = {r['symbol']: r['name'] for r in ast.literal_eval(
        _assigned(_parse(root, 'data', 'amino_acids.py'), 'amino_acid_records'))}
    state = _function(expr, 'get_flagella_initial_state')
    counts = {}                                  # molecules[nucleotide] = 5000000, molecules[amino_acid] = 1000000
    for loop in (n for n in ast.walk(state) if isinstance(n, ast.For)):
        counts[loop.target.id] = ast.literal_eval(loop.body[0].value)
    molecules = {m: counts['nucleotide'] for m in nucleotides.values()}
    molecules.update({m: counts['amino_acid'] for m in amino_acids.values()})
    proteins = None
    for d in (n for n in ast.walk(state) if isinstance(n, ast.Dict)):
        if any(isinstance(k, ast.Constant) and k.value == 'endoRNAse' for k in d.keys):
            proteins = {(_literal(k, names)): ast.literal_eval(v) for k, v in zip(d.keys, d.values)}
    path = write('flagella_degradation.json', {
        'source': 'vivarium/compartments/flagella_expression.py:119-128,318-349; '
                  'vivarium/data/chromosomes/flagella_chromosome.py (genes)',
        'catalytic_rates': rates,
        'michaelis_constants': {'transcripts': kms},
        'initial_state': {'molecules': molecules, 'transcripts': {o: 0 for o in operons}, 'proteins': proteins},
    })
    print(path, len(operons), 'operons,', len(proteins), 'proteins')
    deg = _parse(root, 'processes', 'degradation.py')
    km = {'DEFAULT_TRANSCRIPT_DEGRADATION_KM': ast.literal_eval(_assigned(deg, 'DEFAULT_TRANSCRIPT_DEGRADATION_KM'))}
    toy = _literal(_assigned(deg, 'TOY_CONFIG'), km)
    # test_rna_degradation: 10 of every protein, molecule and transcript, ATP 100000, time_step 1.0, 10 s
    toy['initial_state'] = {'proteins': {p: 10 for p in toy['catalytic_rates']},
                            'molecules': dict({m: 10 for m in list(nucleotides.values()) + ['ADP']}, ATP=100000),
                            'transcripts': {t: 10 for t in toy['sequences']}}
    toy['time_step'], toy['total_time'] = 1.0, 10
    toy['source'] = 'vivarium/processes/degradation.py:30-50,185-207'
    print(write('toy_degradation.json', toy))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
