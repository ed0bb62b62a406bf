"""The `plonk` package's place among the import layers ("Layers of the Python package": layer 11), read off
the source with ast as tests/test_layering_cpu.py reads the flat modules: nothing of the package is imported here."""
import ast
import pathlib

PACKAGE = pathlib.Path(__file__).resolve().parent.parent / "octopuszk_amd"
PLONK = PACKAGE / "plonk"
# what the subpackage may import of the package above it, at any level of nesting
ALLOWED = {"kzg", "vectors", "wire", "transcript", "fft", "lib", "device"}


def _relative_imports(path):
    """(level, first module name) of every relative import statement of a file, function-local ones included"""
    out = []
    for node in ast.walk(ast.parse(path.read_text())):
        if isinstance(node, ast.ImportFrom) and node.level >= 1:
            names = [alias.name for alias in node.names] if node.module is None else [node.module.split(".")[0]]
            out += [(node.level, name) for name in names]
    return out


def test_the_package_is_there_and_flat_modules_stay_flat():
    files = {p.name for p in PLONK.glob("*.py")}
    assert "__init__.py" in files and files <= {"__init__.py", "circuit.py", "protocol.py"}
    assert not (PACKAGE / "plonk.py").exists()


def test_plonk_imports_only_the_layers_below():
    own = {p.stem for p in PLONK.glob("*.py")} - {"__init__"}
    seen = set()
    for path in sorted(PLONK.glob("*.py")):
        for level, name in _relative_imports(path):
            if level == 1:
                assert name in own, "%s imports .%s, which is no module of the plonk package" % (path.name, name)
            else:
                assert level == 2 and name in ALLOWED, "%s imports %s%s" % (path.name, "." * level, name)
                seen.add(name)
        for node in ast.walk(ast.parse(path.read_text())):
            if isinstance(node, ast.Import):
                assert not any(alias.name.startswith("octopuszk_amd") for alias in node.names), path.name
            if isinstance(node, ast.ImportFrom) and node.level == 0:
                assert not (node.module or "").startswith("octopuszk_amd"), path.name
    assert "kzg" in seen


def test_no_flat_module_imports_plonk():
    for path in sorted(PACKAGE.glob("*.py")):
        for level, name in _relative_imports(path):
            assert name != "plonk", "%s imports the plonk package" % path.name
        for node in ast.walk(ast.parse(path.read_text())):
            if isinstance(node, ast.Import):
                assert not any("plonk" in alias.name for alias in node.names), path.name
            if isinstance(node, ast.ImportFrom) and node.level == 0:
                assert "plonk" not in (node.module or ""), path.name


def test_design_names_the_layer():
    text = (PACKAGE.parent / "DESIGN.md").read_text()
    assert "layer 11: the `plonk` package" in text
