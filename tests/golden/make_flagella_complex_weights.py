"""Writes flagella_complex_weights.json: the molecular weights of the flagella agent's complexes.

    python tests/golden/make_flagella_complex_weights.py <reference root>

Read from the reference's data tables with ``ast`` (nothing of the reference is imported):

* ``molecular_weight``: vivarium/data/molecular_weight.py restricted to the ``complex_ids`` of
  flagella_complexation.json (the entries marked "from stoichiometry" there).  A complex the
  table does not name has no weight, as in the reference (complexation.py:84-97).

flagella_translation.json already holds the same table's entries for the translated proteins.
Nothing here is imported at test time; tests read only the written file.
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(root):
    complexes = json.load(open(os.path.join(HERE, 'flagella_complexation.json')))['complex_ids']
    weights = {}
    tree = ast.parse(open(os.path.join(root, 'vivarium', 'data', 'molecular_weight.py')).read())
    for d in (n for n in ast.walk(tree) if isinstance(n, ast.Dict)):
        for k, v in zip(d.keys, d.values):
            if isinstance(k, ast.Constant) and isinstance(v, ast.Constant) and isinstance(v.value, (int, float)):
                weights.setdefault(k.value, float(v.value))
    out = {'source': 'vivarium/data/molecular_weight.py; vivarium/processes/complexation.py:84-97',
           'molecular_weight': {c: weights[c] for c in complexes if c in weights}}
    path = os.path.join(HERE, 'flagella_complex_weights.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(path, len(out['molecular_weight']), 'weights')


if __name__ == '__main__':
    main(sys.argv[1])
