"""Generate tests/golden/gradients.npz from the REFERENCE's own gradient code (TEST FIXTURE
GENERATOR; run where the reference tree exists -- the GPU tests only read the committed .npz).

vivarium/processes/diffusion_field.py and static_field.py do not import here (pint and the
plotting stack are missing), but the three pieces wanted are self-contained, so this script
reads the files' ASTs and evaluates only them, unchanged, with numpy:

* ``gaussian(deviation, distance)``                    diffusion_field.py:39-40
* ``make_gradient(gradient, n_bins, size)``            diffusion_field.py:42-206
* ``StaticField.get_concentration(self, location)``    static_field.py:92-119, compiled as a
  module-level function and called with a stand-in ``self`` that has ``gradient`` and ``bounds``.

No reference source is copied into the repository.  The reference is untrusted input, so
nothing of it runs before an AST whitelist has passed it (``_check``): assignments, ``for``
over ``range`` / ``.items()``, ``if``, ``return``, arithmetic, comparisons, subscripts, list
and dict displays, docstrings, calls of the few numpy functions named in ``_NP``, of
``range``, ``gaussian`` and of ``.get`` / ``.items``, and attributes ``gradient`` / ``bounds``.
The pieces are then evaluated with ``range`` as the only builtin.

Recorded (arrays and names only), for the gradients of tests/static_field_ref.py:

* ``grid_<type>``    [2, 5, 7]: make_gradient of all four types on 5 x 7 bins over (10, 21),
  molecules ``a`` and ``b``;
* ``points``         [2, 64] locations on (1000, 3000);
* ``points_<type>``  [2, 64]: get_concentration of the three field types there.

    python tests/golden/make_gradient_ref.py
"""

from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np

REF = '/root/reference/vivarium/processes'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gradients.npz')

_NP = {'exp', 'power', 'sqrt', 'ones', 'zeros', 'full', 'float64'}
_ATTRS = _NP | {'get', 'items', 'gradient', 'bounds'}
_CALLABLE_NAMES = {'range', 'gaussian'}
_ALLOWED = (ast.FunctionDef, ast.arguments, ast.arg, ast.Assign, ast.AugAssign, ast.For, ast.If, ast.Return, ast.Expr,
            ast.Compare, ast.Eq, ast.BinOp, ast.UnaryOp, ast.Add, ast.Sub, ast.Mult, ast.Div, ast.Pow, ast.USub,
            ast.Name, ast.Load, ast.Store, ast.Constant, ast.Subscript, ast.Call, ast.Attribute, ast.keyword,
            ast.Dict, ast.List, ast.Tuple)


def _check(fn):
    for n in ast.walk(fn):
        if not isinstance(n, _ALLOWED):
            raise ValueError('%s: disallowed node %s' % (fn.name, type(n).__name__))
        if isinstance(n, ast.Attribute):
            root = n.value
            while isinstance(root, ast.Subscript):
                root = root.value
            if isinstance(root, ast.Attribute) and isinstance(root.value, ast.Name) and root.value.id == 'self':
                root = root.value           # self.gradient['molecules'].items()
            if n.attr not in _ATTRS or not isinstance(root, ast.Name) or ((root.id == 'np') != (n.attr in _NP)):
                raise ValueError('%s: disallowed attribute %s' % (fn.name, ast.unparse(n)))
        if isinstance(n, ast.Call):
            f = n.func
            if not (isinstance(f, ast.Attribute) or (isinstance(f, ast.Name) and f.id in _CALLABLE_NAMES)):
                raise ValueError('%s: disallowed call %s' % (fn.name, ast.unparse(n)))
        if isinstance(n, ast.keyword) and n.arg != 'dtype':
            raise ValueError('%s: disallowed keyword %s' % (fn.name, n.arg))
        if isinstance(n, ast.Constant) and not isinstance(n.value, (int, float, str)):
            raise ValueError('%s: disallowed constant %r' % (fn.name, n.value))
        if isinstance(n, ast.Expr) and not isinstance(n.value, ast.Constant):   # docstrings only
            raise ValueError('%s: disallowed statement %s' % (fn.name, ast.unparse(n)))


def _functions(path, names, cls=None):
    tree = ast.parse(open(path).read(), path)
    body = tree.body if cls is None else next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return [next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name) for name in names]


def pieces():
    """(gaussian, make_gradient, get_concentration) of the reference."""
    fns = (_functions(os.path.join(REF, 'diffusion_field.py'), ['gaussian', 'make_gradient']) +
           _functions(os.path.join(REF, 'static_field.py'), ['get_concentration'], cls='StaticField'))
    ns = {'__builtins__': {'range': range}, 'np': np}
    for fn in fns:
        _check(fn)
        fn.decorator_list = []
        exec(compile(ast.Module(body=[fn], type_ignores=[]), REF, 'exec'), ns)
    return ns['gaussian'], ns['make_gradient'], ns['get_concentration']


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import static_field_ref as sref
    _, make_gradient, get_concentration = pieces()
    out = {'molecules': np.array(['a', 'b']), 'types': np.array(sref.TYPES), 'points': sref.points(),
           'grid_bins': np.array(sref.GRID_BINS), 'grid_bounds': np.array(sref.GRID_BOUNDS, dtype=np.float64),
           'point_bounds': np.array(sref.POINT_BOUNDS, dtype=np.float64)}
    for kind in sref.TYPES:
        fields = make_gradient(sref.GRID[kind], list(sref.GRID_BINS), list(sref.GRID_BOUNDS))
        out['grid_' + kind] = np.stack([fields['a'], fields['b']])
    for kind in sref.FIELD_TYPES:
        me = types.SimpleNamespace(gradient=sref.POINTS[kind], bounds=list(sref.POINT_BOUNDS))
        rows = [get_concentration(me, [float(x), float(y)]) for x, y in out['points'].T]
        out['points_' + kind] = np.array([[r['a'] for r in rows], [r['b'] for r in rows]], dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
