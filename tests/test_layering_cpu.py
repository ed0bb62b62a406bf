"""The package's import layers ("Layers of the Python package"), read off the source with ast: nothing of
the package is imported here."""
import ast
import pathlib

PACKAGE = pathlib.Path(__file__).resolve().parent.parent / "octopuszk_amd"

# lowest first; a module imports, at module level, only from layers below its own
LAYERS = (
    ("lib", "build", "keyfile", "transcript"),
    ("fft", "wire"),
    ("device",),
    ("codec", "pairing"),
    ("vectors",),
    ("r1cs_to_qap", "fixed_base_msm", "variable_base_msm", "distributed"),
    ("bace",),
    ("zksnark",),
    ("ceremony", "srs"),
    ("kzg",),
)
LAYER = {name: i for i, names in enumerate(LAYERS) for name in names}
# the two imports inside a layer, both one-way: wire takes the modulus FR from fft, and the phase-1 ceremony (srs)
# proves and encodes with the phase-2 ceremony's receipt helpers
WITHIN_LAYER = {("wire", "fft"), ("srs", "ceremony")}
# (module, function, imported module): each points upward from a convenience method, or is one of device.py,
# distributed.py and variable_base_msm.py's own
LOCAL_IMPORTS = {
    ("zksnark", "ProvingKey.contribute", "ceremony"),
    ("zksnark", "ProvingKey.verify_contribution", "ceremony"),
    ("zksnark", "setup_from_srs", "srs"),
    ("device", "groth16_combine", "zksnark"),
    ("distributed", "gpu_var_msm", "device"),
    ("distributed", "gpu_var_double_msm", "device"),
    ("variable_base_msm", "batched_serial_msm", "device"),
}


def _targets(node):
    """the modules of this package a relative import statement names"""
    if not isinstance(node, ast.ImportFrom) or node.level != 1:
        return []
    if node.module is None:                      # from . import a, b
        return [alias.name for alias in node.names]
    return [node.module.split(".")[0]]           # from .a import x


def _imports():
    """(module-level, function-local) relative imports of every module: sets of (module, enclosing scope, target)"""
    top, local = set(), set()
    for path in sorted(PACKAGE.glob("*.py")):
        def visit(node, scope, in_function):
            for child in ast.iter_child_nodes(node):
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    visit(child, scope + (child.name,), True)
                elif isinstance(child, ast.ClassDef):
                    visit(child, scope + (child.name,), in_function)
                else:
                    for target in _targets(child):
                        (local if in_function else top).add((path.stem, ".".join(scope), target))
                    visit(child, scope, in_function)

        visit(ast.parse(path.read_text()), (), False)
    return top, local


def test_every_module_has_a_layer():
    modules = {p.stem for p in PACKAGE.glob("*.py")} - {"__init__"}
    assert modules == set(LAYER), modules ^ set(LAYER)
    assert sum(len(names) for names in LAYERS) == len(LAYER)        # no module in two layers


def test_module_level_imports_go_down():
    edges = {(module, target) for module, _, target in _imports()[0] if module != "__init__"}
    assert WITHIN_LAYER <= edges
    for module, target in sorted(edges):
        assert target in LAYER, "%s imports .%s, which is no module of the table" % (module, target)
        if (module, target) in WITHIN_LAYER:
            assert LAYER[target] == LAYER[module] and (target, module) not in edges
        else:
            assert LAYER[target] < LAYER[module], "%s (layer %d) imports %s (layer %d) at module level" % (
                module, LAYER[module] + 1, target, LAYER[target] + 1)


def test_function_local_imports_are_the_allowed_ones():
    _, local = _imports()
    assert local == LOCAL_IMPORTS, sorted(local ^ LOCAL_IMPORTS)
