"""What octopuszk_amd/build.py reads out of the depfiles that hipcc writes beside every object (-MD -MF): the
prerequisites that lie inside the repository, and from them whether an object is stale.  The parser runs on text
written into a temporary directory; no file of the repository is touched.  Where a built tree is present, the
dependency lists of the kzg and plonk units are also checked for the two headers every Fr kernel is built from."""
import os

import pytest

from octopuszk_amd import build as b


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


@pytest.fixture
def tree(tmp_path):
    """a root with two headers and a header whose directory has a space in its name, and an object beside them"""
    root = tmp_path / "repo"
    (root / "csrc").mkdir(parents=True)
    (root / "my include").mkdir()
    for rel in ("csrc/a.hip", "csrc/a.cuh", "csrc/b.cuh", "my include/api.h"):
        _write(root / rel, "")
    obj = _write(root / "a.hip.o", "")
    return root, obj


def _depfile(root, obj):
    return (f"{obj}: {root}/csrc/a.hip \\\n"
            f"  /opt/rocm/include/hip/hip_runtime.h \\\n"
            f"  /usr/include/c++/11/cmath {root}/csrc/a.cuh \\\n"
            f"  {root}/csrc/../csrc/b.cuh \\\n"
            f"  {str(root).replace(' ', chr(92) + ' ')}/my\\ include/api.h\n")


def test_continuations_escaped_spaces_and_system_headers(tree):
    root, obj = tree
    _write(obj + ".d", _depfile(root, obj))
    want = [os.path.join(root, rel) for rel in ("csrc/a.hip", "csrc/a.cuh", "csrc/b.cuh", "my include/api.h")]
    assert b.depfile_deps(obj + ".d", str(root)) == want


def test_a_rule_on_one_line_and_an_empty_rule(tree):
    root, obj = tree
    _write(obj + ".d", f"{obj}: {root}/csrc/a.hip {root}/csrc/a.cuh\n\n{root}/csrc/a.cuh:\n")
    assert b.depfile_deps(obj + ".d", str(root)) == [os.path.join(root, "csrc/a.hip"), os.path.join(root, "csrc/a.cuh")]


def test_a_missing_depfile_means_stale(tree):
    root, obj = tree
    src = os.path.join(root, "csrc/a.hip")
    assert b.depfile_deps(obj + ".d", str(root)) is None
    assert b.object_is_stale(obj, src, str(root))


def test_stale_follows_the_repository_files_of_the_depfile(tree):
    root, obj = tree
    src = os.path.join(root, "csrc/a.hip")
    _write(obj + ".d", _depfile(root, obj))
    t = os.path.getmtime(obj)
    for rel in ("csrc/a.hip", "csrc/a.cuh", "csrc/b.cuh", "my include/api.h"):
        os.utime(os.path.join(root, rel), (t - 10, t - 10))
    assert not b.object_is_stale(obj, src, str(root))
    assert b.object_is_stale(obj, os.path.join(root, "elsewhere/a.hip"), str(root))   # written for a tree in another place
    os.utime(os.path.join(root, "my include/api.h"), (t + 10, t + 10))   # the last one listed, behind the escaped space
    assert b.object_is_stale(obj, src, str(root))
    os.utime(os.path.join(root, "my include/api.h"), (t - 10, t - 10))
    os.remove(os.path.join(root, "csrc/b.cuh"))                          # a header that is gone
    assert b.object_is_stale(obj, src, str(root))
    os.remove(obj)                                                       # no object
    _write(os.path.join(root, "csrc/b.cuh"), "")
    assert b.object_is_stale(obj, src, str(root))


@pytest.mark.parametrize("unit", ["kzg.hip", "plonk.hip"])
def test_built_fr_units_depend_on_the_shared_headers(unit):
    dep = os.path.join(b.HERE, "_obj", unit + ".o.d")
    if not os.path.exists(dep):
        pytest.skip("no built tree: %s is not there" % os.path.relpath(dep, b.ROOT))
    # (by name, over every prerequisite: the depfile holds the paths of the place where the tree was built)
    names = {os.path.basename(d) for d in b.depfile_deps(dep, os.sep)}
    assert unit in names
    for header in ("fr_rows.cuh", "fr_tables.cuh"):
        assert header in names
