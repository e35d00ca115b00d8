"""Host-side checks of the `uc_nerf_amd.ops` package's surface.  No GPU, no library: every name the single-file module had (recorded in
golden/ops_surface.txt before it was split) still resolves on the package, each is defined in exactly one submodule, the module state stays in
its home module, and a setter's change reaches the readers in the other modules."""
import ast
import importlib
import os
import pkgutil

import pytest

from uc_nerf_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("_backward_mode", "_split_operand", "_guard_words", "_loss_words", "_BRT_PREPARED")
SUBMODULES = sorted(m.name for m in pkgutil.iter_modules(ops.__path__))


@pytest.fixture(scope="module")
def surface():
    with open(os.path.join(ROOT, "tests", "golden", "ops_surface.txt")) as f:
        return f.read().split()


def _tree(module):
    with open(os.path.join(ops.__path__[0], module + ".py")) as f:
        return ast.parse(f.read())


def _top_level_names(tree):
    """(names bound by def / class / assignment at module level, the nodes that bind them)."""
    names, nodes = [], []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.append(node.name)
            nodes.append(node)
        elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            targets = node.targets if isinstance(node, ast.Assign) else [node.target]
            names += [n.id for t in targets for n in ast.walk(t) if isinstance(n, ast.Name)]
            nodes.append(node)
    return names, nodes


def test_every_recorded_name_resolves_on_the_package(surface):
    assert len(surface) == len(set(surface)) >= 100
    missing = [n for n in surface if not hasattr(ops, n)]
    assert not missing, missing


def test_state_is_not_an_attribute_of_the_package(surface):
    assert not [n for n in STATE if hasattr(ops, n)]
    assert not set(STATE) & set(surface)
    homes = {n: [m for m in SUBMODULES if n in _top_level_names(_tree(m))[0]] for n in STATE}
    assert all(len(h) == 1 for h in homes.values()), homes


def test_each_name_has_one_home_and_the_package_file_defines_nothing(surface):
    init_names, init_nodes = _top_level_names(_tree("__init__"))
    assert not init_names and not init_nodes
    assert not [n for n in ast.walk(_tree("__init__")) if isinstance(n, (ast.FunctionDef, ast.Lambda, ast.ClassDef))]
    defined = {m: _top_level_names(_tree(m))[0] for m in SUBMODULES}
    for name in surface:
        homes = [m for m in SUBMODULES if name in defined[m]]
        assert len(homes) == 1 and defined[homes[0]].count(name) == 1, (name, homes)
        obj = getattr(ops, name)
        assert obj is getattr(importlib.import_module("uc_nerf_amd.ops." + homes[0]), name), name
        if not isinstance(obj, (tuple, dict)):
            assert obj.__module__ == "uc_nerf_amd.ops." + homes[0], (name, obj.__module__)


def test_setters_reach_their_readers():
    old = ops.backward_mode()
    try:
        ops.set_backward_mode("layerwise")
        assert ops.backward_mode() == "layerwise" and ops.network._backward_mode == ops.BACKWARD_MODES["layerwise"]
        ops.set_backward_mode("chain")
        assert ops.backward_mode() == "chain"
    finally:
        ops.set_backward_mode(old)
    old = ops.split_operand()
    try:
        for kind in ops.SPLIT_OPERANDS:
            ops.set_split_operand(kind)
            assert ops.split_operand() == kind and ops.network._split_operand == ops.SPLIT_OPERANDS[kind]
    finally:
        ops.set_split_operand(old)
    # no module but the modes' home may hold a copy of either integer: a copy goes stale with the next set_*()
    for m in SUBMODULES:
        if m == "network":
            continue
        tree = _tree(m)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                assert not {a.name for a in node.names} & {"_backward_mode", "_split_operand"}, (m, node.lineno)
        for node in _top_level_names(tree)[1]:
            if not isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                used = {n.attr if isinstance(n, ast.Attribute) else getattr(n, "id", None) for n in ast.walk(node)}
                assert not used & {"_backward_mode", "_split_operand"}, (m, node.lineno)
    with open(os.path.join(ops.__path__[0], "render.py")) as f:
        assert "network._backward_mode" in f.read()      # (read through the module, at call time)
