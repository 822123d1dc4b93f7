"""Generate tests/golden/flagella_translation.json (run once where the reference tree is).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flagella_translation.py REFERENCE_ROOT

The translation config of the reference's flagella agent
(vivarium/compartments/flagella_expression.py:110-117) is built by FlagellaChromosome
(vivarium/data/chromosomes/flagella_chromosome.py:333-365), which does not import without
``pint``, so this script reads the data out of the two source files with ``ast`` (nothing of
the reference is executed):

* ``transcripts``: the (operon, product) keys in the reference's order (its ``genes`` dict);
* ``transcript_affinities``: min_tr_affinity * tr_affinity_scaling.get(product, 1) per key;
* ``elongation_rate`` 22 and ``polymerase_occlusion`` 50;
* ``molecular_weight`` of every product (vivarium/data/molecular_weight.py).

The protein sequences are NOT in the file: the reference reads them from
data/flat/wcEcoli_proteins.tsv through its KnowledgeBase, and that table is not part of the
reference tree this was generated from.  ``estimated_length`` is round(molecular weight /
110 Da), the mean residue mass, so that a config of the right size can be synthesised
(lens_amd.configs.flagella_translation); pass real sequences there where they are at hand.

Nothing here is imported at test time; tests read only the written file.
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN_RESIDUE_DA = 110.0


def _find(tree, test):
    return [node for node in ast.walk(tree) if test(node)]


def main(root):
    src = open(os.path.join(root, 'vivarium', 'data', 'chromosomes', 'flagella_chromosome.py')).read()
    tree = ast.parse(src)
    genes = None
    for d in _find(tree, lambda n: isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and k.value == 'genes' and isinstance(v, ast.Dict):
                genes = ast.literal_eval(v)
    scaling = [ast.literal_eval(n.value) for n in _find(tree, lambda n: isinstance(n, ast.Assign))
               if isinstance(n.targets[0], ast.Name) and n.targets[0].id == 'tr_affinity_scaling'][0]
    minimum = [ast.literal_eval(n.args[1]) for n in _find(tree, lambda n: isinstance(n, ast.Call))
               if len(n.args) == 2 and isinstance(n.args[0], ast.Constant) and n.args[0].value == 'min_tr_affinity'][0]
    expr = ast.parse(open(os.path.join(root, 'vivarium', 'compartments', 'flagella_expression.py')).read())
    translation = None
    for d in _find(expr, lambda n: isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and k.value == 'translation' and isinstance(v, ast.Dict):
                named = {kk.value: vv for kk, vv in zip(v.keys, v.values) if isinstance(kk, ast.Constant)}
                if 'elongation_rate' in named:
                    translation = {name: ast.literal_eval(named[name])
                                   for name in ('elongation_rate', 'polymerase_occlusion')}
    weights = {}
    mw = ast.parse(open(os.path.join(root, 'vivarium', 'data', 'molecular_weight.py')).read())
    for d in _find(mw, lambda n: isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and isinstance(v, ast.Constant) and isinstance(v.value, (int, float)):
                weights.setdefault(k.value, float(v.value))
    transcripts = [[operon, product] for operon, products in genes.items() for product in products]
    products = sorted({p for _, p in transcripts})
    out = {
        'source': 'vivarium/data/chromosomes/flagella_chromosome.py:58-75,333-365; '
                  'vivarium/compartments/flagella_expression.py:110-117; vivarium/data/molecular_weight.py',
        'transcripts': transcripts,
        'transcript_affinities': [minimum * scaling.get(product, 1) for _, product in transcripts],
        'elongation_rate': translation['elongation_rate'],
        'polymerase_occlusion': translation['polymerase_occlusion'],
        'molecular_weight': {p: weights[p] for p in products if p in weights},
        'estimated_length': {p: int(round(weights[p] / MEAN_RESIDUE_DA)) for p in products if p in weights},
        'sequences': None,
    }
    path = os.path.join(HERE, 'flagella_translation.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(path, len(transcripts), 'transcripts,', len(out['estimated_length']), 'lengths')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
