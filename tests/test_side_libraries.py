"""CPU tests of the side libraries' registries, one case per row of __graft_entry__.SIDE_LIBRARIES: the binding's table
(vggsfm_amd/_lib_<name>.py) against the header beside the source type by type, both against the dynamic symbols of the shared
object, the loud failure without it, and -- over all rows at once -- that the ten libraries are disjoint, closed sets and that
the table of rows is complete.  What only one library has (pinned prototypes, #define constants) is in its test_*_host.py.
No kernel is called here."""
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

import __graft_entry__ as G
from tests.test_c_abi import _parse_header, _prefix, _table_kinds
from vggsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "vggsfm_amd")
INCLUDE = os.path.join(ROOT, "include")
DIRECTORIES = [directory for directory, _ in G.SIDE_LIBRARIES]
BINDINGS = {directory: importlib.import_module("vggsfm_amd." + binding) for directory, binding in G.SIDE_LIBRARIES}
# prefix and number of entries per library, build_arch included: closed, counted sets, like COUNTS of tests/test_c_abi.py
PREFIXES = {"klt": "vggk_", "mvs": "vggm_", "selftest": "vggs_", "fuse": "vggf_", "patchmatch": "vggr_", "tsdf": "vggv_",
            "raster": "vggz_", "nn": "vggn_", "icp": "vggi_"}
COUNTS = {"klt": 6, "mvs": 3, "selftest": 2, "fuse": 3, "patchmatch": 5, "tsdf": 5, "raster": 4, "nn": 9, "icp": 6}
SHORT_NAMES = {"patchmatch": "pm"}                     # libvggsfm_amd_<directory>.so but for this one
# the product module of a library and the name under which it imports the binding (the self-tests have none)
PRODUCTS = {"klt": ("klt.py", "K"), "mvs": ("mvs.py", "M"), "fuse": ("fusion.py", "F"), "patchmatch": ("patchmatch.py", "PM"),
            "tsdf": ("meshing.py", "T"), "raster": ("render.py", "Z"), "nn": ("nearest.py", "N"), "icp": ("registration.py", "I")}
# vggs_ is also the prefix of the Sim(3) entries of the main library (include/vggsfm_amd_sim3.h); the names still differ
PREFIX_SHARED_WITH_INCLUDE = {"selftest"}


def _symbols(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r" T (vgg[a-z]*_\w+)$", nm, flags=re.M))


@pytest.mark.parametrize("directory", DIRECTORIES)
def test_header_and_table_agree(directory):
    """The table's rows against the prototypes type by type, in the header's order; a counted set under one prefix, opened by
    <prefix>build_arch; the header beside the source and the prefix unknown to include/."""
    B = BINDINGS[directory]
    functions, structs = _parse_header(open(B.HEADER_PATH).read())
    table = _table_kinds(B.SIGNATURES)
    assert list(table) == list(functions) and not structs                   # same names, in the header's order
    for name in functions:
        assert table[name] == functions[name], name
    assert len(functions) == COUNTS[directory]
    prefix = PREFIXES[directory]
    assert {_prefix(name) for name in functions} == {prefix}
    assert list(functions.items())[0] == (prefix + "build_arch", ("pointer", []))
    assert os.path.dirname(B.HEADER_PATH) == os.path.join(PACKAGE, "csrc", directory) and os.path.basename(B.HEADER_PATH) == B.HEADER
    assert B.HEADER not in os.listdir(INCLUDE)
    if directory not in PREFIX_SHARED_WITH_INCLUDE:
        for name in os.listdir(INCLUDE):
            assert prefix not in open(os.path.join(INCLUDE, name)).read(), name


@pytest.mark.parametrize("directory", DIRECTORIES)
def test_library_exports_and_binds_the_table(directory):
    """The shared object's defined dynamic symbols are exactly the table; it loads, was built for gfx950, and every bound
    function carries its row's types."""
    B = BINDINGS[directory]
    assert B.LIB_PATH == os.path.join(PACKAGE, f"libvggsfm_amd_{SHORT_NAMES.get(directory, directory)}.so")
    assert os.path.exists(B.LIB_PATH), "run __graft_entry__.build() first"
    assert _symbols(B.LIB_PATH) == set(B.SIGNATURES)
    L = B.lib()
    assert getattr(L, PREFIXES[directory] + "build_arch")() == b"gfx950"
    for name, (restype, argtypes) in B.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


@pytest.mark.parametrize("directory", DIRECTORIES)
def test_import_without_the_library_fails_loudly(directory, tmp_path):
    """A copy of the package holding only _lib.py and the binding: lib() raises, naming the missing file and the build
    command; there is no fallback.  And the product module loads the library when it is imported."""
    binding = BINDINGS[directory].__name__.rpartition(".")[2]
    pkg = tmp_path / "vggsfm_amd"
    pkg.mkdir()
    for name in ("_lib.py", binding + ".py"):
        shutil.copy(os.path.join(PACKAGE, name), pkg / name)
    (pkg / "__init__.py").write_text("")
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            f"try:\n    import vggsfm_amd.{binding} as T\n    T.lib()\nexcept RuntimeError as e:\n    print('RuntimeError:', e)\n"
            "else:\n    print('loaded')\n")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("RuntimeError:") and os.path.basename(BINDINGS[directory].LIB_PATH) + " is missing" in out.stdout \
        and f"make -C vggsfm_amd/csrc/{directory}`" in out.stdout and "no CPU or eager fallback" in out.stdout, out.stdout
    if directory in PRODUCTS:
        module, alias = PRODUCTS[directory]
        text = open(os.path.join(PACKAGE, module)).read()
        assert f"from . import {binding} as {alias}\n" in text and f"\n_L = {alias}.lib()" in text, module


def test_the_libraries_are_disjoint_closed_sets():
    """Ten libraries, the main one among them: pairwise distinct prefixes among the side libraries, pairwise disjoint tables,
    every one exporting its table in the table's order."""
    tables = {"main": _lib, **BINDINGS}
    prefixes = [PREFIXES[directory] for directory in BINDINGS]
    assert len(set(prefixes)) == len(prefixes) == 9
    assert [p for p in prefixes if p in {_prefix(name) for name in _lib.SIGNATURES}] == ["vggs_"]     # (the Sim(3) entries)
    names = [name for B in tables.values() for name in B.SIGNATURES]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    for which, B in tables.items():
        assert B.EXPORTED == list(B.SIGNATURES), which
        assert _symbols(B.LIB_PATH) == set(B.SIGNATURES), which             # none took another's translation unit in


def test_the_table_of_rows_is_complete():
    """Every directory under csrc/ with a Makefile and every _lib_*.py is a row, and the other way round."""
    csrc = os.path.join(PACKAGE, "csrc")
    assert sorted(DIRECTORIES) == sorted(d for d in os.listdir(csrc) if os.path.exists(os.path.join(csrc, d, "Makefile")))
    assert sorted(binding + ".py" for _, binding in G.SIDE_LIBRARIES) == \
        sorted(n for n in os.listdir(PACKAGE) if re.fullmatch(r"_lib_\w+\.py", n))
    assert len(G.SIDE_LIBRARIES) == len(set(DIRECTORIES)) == 9 and set(COUNTS) == set(PREFIXES) == set(DIRECTORIES) and set(PRODUCTS) < set(COUNTS)
    assert DIRECTORIES == ["klt", "mvs", "selftest", "fuse", "patchmatch", "tsdf", "raster", "nn", "icp"]       # the build order


def test_the_dense_libraries_share_their_limits():
    """The refinement starts from the stereo's sweep and the fusion reads both: one MAX_SOURCES, one MAX_RADIUS (each
    library's host test compares its own value with its header)."""
    mvs, fuse, pm = BINDINGS["mvs"], BINDINGS["fuse"], BINDINGS["patchmatch"]
    assert fuse.MAX_SOURCES == pm.MAX_SOURCES == mvs.MAX_SOURCES and pm.MAX_RADIUS == mvs.MAX_RADIUS
