"""Where the Python side of the kernels lives, without a GPU: ``ops`` is one module that holds the CTR core and re-exports
the leaf families of ``torch_rechub_amd/_families`` under the names callers have always used; the families and ``_opcore``
never import ``ops``, so each imports on its own and in either order."""
import ast
import importlib
import os
import pkgutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "torch_rechub_amd")
FAMILIES = sorted(m.name for m in pkgutil.iter_modules([os.path.join(PKG, "_families")]))


def imports_of(path):
    """(level, module, names) of every import statement in a file, the late ones inside functions included."""
    with open(path) as f:
        tree = ast.parse(f.read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            out.append((node.level, node.module or "", [a.name for a in node.names], node.lineno))
        elif isinstance(node, ast.Import):
            out += [(0, a.name, [], node.lineno) for a in node.names]
    return out


def reexports():
    """{family: names} of the ``from ._families.<family> import ...`` statements of ops.py."""
    out = {}
    for level, module, names, _ in imports_of(os.path.join(PKG, "ops.py")):
        if level == 1 and module.startswith("_families."):
            out.setdefault(module[len("_families."):], []).extend(names)
    return out


def test_there_is_a_module_per_family_and_ops_reexports_each():
    assert FAMILIES == sorted(["interest", "sine", "rq", "hstu", "hllm", "session", "topk", "ivf", "sasrec", "twotower", "t5attn",
                               "beam", "cin", "metric"])
    assert sorted(reexports()) == FAMILIES
    assert all("*" not in names for names in reexports().values())


def test_each_family_imports_before_ops_in_a_fresh_interpreter():
    """One child per family, all started at once: the family module first, then ops."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    children = {}
    for fam in FAMILIES:
        code = f"import torch_rechub_amd._families.{fam}\nimport torch_rechub_amd.ops\n"
        children[fam] = subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                         stderr=subprocess.STDOUT)
    failed = {}
    for fam, child in children.items():
        out, _ = child.communicate()
        if child.returncode != 0:
            failed[fam] = out.decode(errors="replace")[-2000:]
    assert not failed, failed


@pytest.mark.parametrize("name", ["_opcore"] + ["_families." + f for f in FAMILIES])
def test_no_family_reaches_for_ops(name):
    """A family imports _lib, _opcore and a sibling family at most (the package's __init__ imports ops long before any
    family, so only the source can show that a family would import alone)."""
    package = name.split(".")[:-1]  # below torch_rechub_amd
    allowed = {"_lib", "_opcore", "models"}  # models: the late imports of no_kernel and of rqvae's Sinkhorn helpers, in functions
    if package:
        allowed.add("_families")
    for level, module, names, line in imports_of(os.path.join(PKG, *name.split(".")) + ".py"):
        if level == 0:
            assert module.split(".")[0] != "torch_rechub_amd", (name, line)
            continue
        base = package[:len(package) - (level - 1)]
        targets = [base + module.split(".")] if module else [base + [n] for n in names]
        for t in targets:
            assert t[0] in allowed, (name, line, ".".join(t))


@pytest.mark.parametrize("family", FAMILIES)
def test_ops_names_are_the_family_modules_objects(family):
    from torch_rechub_amd import ops
    module = importlib.import_module("torch_rechub_amd._families." + family)
    names = reexports()[family]
    assert names
    for n in names:
        assert getattr(ops, n) is getattr(module, n), n
    public = [n for n in vars(module) if not n.startswith("_") and getattr(vars(module)[n], "__module__", None) == module.__name__]
    assert set(public) <= set(names), sorted(set(public) - set(names))


def test_the_core_helpers_exist_once():
    from torch_rechub_amd import _opcore, ops
    for n in ("_NULL", "_p", "_stream", "require_hip", "_dropout_rng", "_rng_state", "_empty_stub", "_ptr_array", "_int_array"):
        assert getattr(ops, n) is getattr(_opcore, n), n
