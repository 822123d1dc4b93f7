"""Generate tests/golden/flagella_transcription.json and tests/golden/toy_chromosome.json (run once
where the reference tree is).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flagella_transcription.py REFERENCE_ROOT

The transcription config of the reference's flagella agent
(vivarium/compartments/flagella_expression.py:100-108) is built by FlagellaChromosome
(vivarium/data/chromosomes/flagella_chromosome.py:19-331), which does not import without
``pint``, so this script reads the data out of the source files with ``ast`` (nothing of the
reference is executed):

* ``promoters``: the 15 promoters (id, position, direction, sites, terminators) in the
  reference's order, with the site thresholds AFTER ``apply_thresholds(factor_thresholds)``
  (vivarium/states/chromosome.py:204-213, restated below), as magnitudes in mM: fliLp1 / flhDC is
  1e-06, not the 4e-06 written in the promoter;
* ``genes``, ``transcription_factors``;
* ``promoter_affinities`` as [[promoter, state, ...], affinity] pairs (JSON has no tuple keys),
  with ``binary_sum_gates`` (flagella_chromosome.py:301-314) restated below;
* ``elongation_rate`` 50 and ``polymerase_occlusion`` 30.

The E. coli genome (data/flat/Escherichia_coli_str_k_12_substr_mg1655...fa) is NOT in the
reference tree this was generated from, so the file carries no sequence (``sequence``: null);
lens_amd.configs.flagella_transcription draws a seeded random genome over a compact layout
that keeps every promoter's length and direction.

``toy_chromosome.json`` is ``toy_chromosome_config`` (vivarium/data/chromosomes/
toy_chromosome.py), the thresholds as magnitudes in mM, the affinities as pairs as above and the
domains as a list.

Nothing here is imported at test time; tests read only the written files.
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


class _Magnitudes(ast.NodeTransformer):
    """x * units.mM -> x."""

    def visit_BinOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Mult) and isinstance(node.right, ast.Attribute) and node.right.attr == 'mM':
            return node.left
        return node


def _literal(node):
    return ast.literal_eval(ast.fix_missing_locations(_Magnitudes().visit(node)))


def _assigned(tree, name):
    """The value node of the first assignment to ``name`` or ``self.name``."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign):
            target = node.targets[0]
            if (isinstance(target, ast.Name) and target.id == name) or (
                    isinstance(target, ast.Attribute) and target.attr == name):
                return node.value
    raise KeyError(name)


def _entry(node, key):
    for k, v in zip(node.keys, node.values):
        if isinstance(k, ast.Constant) and k.value == key:
            return v
    raise KeyError(key)


def apply_thresholds(promoters, thresholds):
    """Chromosome.apply_thresholds: every site of the promoter that names the factor takes the level."""
    for (promoter, factor), level in thresholds.items():
        found = False
        for site in promoters[promoter]['sites']:
            if factor in site['thresholds']:
                site['thresholds'][factor] = level
                found = True
        if not found:
            raise KeyError((promoter, factor))


def binary_sum_gates(promoter_factors):
    """flagella_chromosome.py:301-314: (p, first, None), (p, None, second) and their sum."""
    affinities = {}
    first, second = list(promoter_factors[list(promoter_factors.keys())[0]].keys())
    for promoter, factors in promoter_factors.items():
        affinities[(promoter, first, None)] = factors[first]
        affinities[(promoter, None, second)] = factors[second]
        affinities[(promoter, first, second)] = factors[first] + factors[second]
    return affinities


def pairs(affinities):
    return [[list(k), v] for k, v in affinities.items()]


def write(name, out):
    path = os.path.join(HERE, name)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    return path


def main(root):
    tree = ast.parse(open(os.path.join(root, 'vivarium', 'data', 'chromosomes', 'flagella_chromosome.py')).read())
    config = _assigned(tree, 'chromosome_config')
    promoters, genes = _literal(_entry(config, 'promoters')), _literal(_entry(config, 'genes'))
    apply_thresholds(promoters, _literal(_assigned(tree, 'factor_thresholds')))
    affinities = _literal(_assigned(tree, 'promoter_affinities'))
    affinities.update(binary_sum_gates(_literal(_assigned(tree, 'flhDC_factors'))))
    for promoter in _literal(_assigned(tree, 'fliA_activated')):
        affinities[(promoter, 'fliA')] = 1.0
    expr = ast.parse(open(os.path.join(root, 'vivarium', 'compartments', 'flagella_expression.py')).read())
    rates = None
    for d in (n for n in ast.walk(expr) if isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and k.value == 'transcription' and isinstance(v, ast.Dict):
                named = {kk.value: vv for kk, vv in zip(v.keys, v.values) if isinstance(kk, ast.Constant)}
                if 'elongation_rate' in named:
                    rates = {name: ast.literal_eval(named[name]) for name in ('elongation_rate', 'polymerase_occlusion')}
    path = write('flagella_transcription.json', {
        'source': 'vivarium/data/chromosomes/flagella_chromosome.py:29-331; '
                  'vivarium/compartments/flagella_expression.py:100-108',
        'promoters': promoters,
        'genes': genes,
        'transcription_factors': _literal(_assigned(tree, 'transcription_factors')),
        'promoter_affinities': pairs(affinities),
        'elongation_rate': rates['elongation_rate'],
        'polymerase_occlusion': rates['polymerase_occlusion'],
        'sequence': None,
    })
    print(path, len(promoters), 'promoters,', len(affinities), 'affinities')
    toy = _literal(_assigned(ast.parse(open(os.path.join(
        root, 'vivarium', 'data', 'chromosomes', 'toy_chromosome.py')).read()), 'toy_chromosome_config'))
    toy['promoter_affinities'] = pairs(toy['promoter_affinities'])
    toy['domains'] = list(toy['domains'].values())
    toy['source'] = 'vivarium/data/chromosomes/toy_chromosome.py'
    print(write('toy_chromosome.json', toy))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
