"""CPU tests of the C-ABI: every public header under include/ against the binding's registry (vggsfm_amd/_lib.py, HEADERS),
type by type, both against the dynamic symbols of the built library, and the ctypes conversions of the registry's parameter
types.  No compute kernel is called here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from vggsfm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
MAIN = "vggsfm_amd.h"
COUNTS = {MAIN: 49, "vggsfm_amd_multiview.h": 7, "vggsfm_amd_essential.h": 4, "vggsfm_amd_pnp.h": 3, "vggsfm_amd_sim3.h": 5,
          "vggsfm_amd_covariance.h": 4}


def _c_kind(decl):
    """Kind of a C parameter or return declaration: "pointer", or the spelling of its value type."""
    decl = " ".join(decl.split())
    if "*" in decl:
        return "pointer"
    return next(k for k in ("unsigned long long", "size_t", "double", "long", "int") if re.match(rf"{k}\b", decl))


def _parse_header(header):
    """-> ({function: (return kind, [parameter kinds])}, {struct: [(field, ctypes type)]}) of the text of a public header."""
    src = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)                  # comments
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)                      # preprocessor lines
    field_type = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    structs = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\} (\w+);", src, flags=re.S):
        fields = structs[name] = []
        for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
            ctype, names = re.fullmatch(r"(.*?[\s*]) ?(\w+(?:, \w+)*)", stmt).groups()
            fields += [(n, ctypes.c_void_p if "*" in ctype else field_type[ctype.strip()]) for n in names.split(", ")]
    src = re.sub(r"typedef struct \{.*?\} \w+;", " ", src, flags=re.S)
    functions = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(vgg[a-z]?_\w+)\s*\(([^)]*)\)\s*;", src):
        assert name not in functions, name
        functions[name] = (_c_kind(ret), [_c_kind(p) for p in params.split(",") if p.strip() != "void"])
    return functions, structs


def _read(header):
    return open(os.path.join(INCLUDE, header)).read()


def _table_kinds(table):
    restype_kind = {ctypes.c_char_p: "pointer", ctypes.c_int: "int", ctypes.c_size_t: "size_t"}
    native = {ctypes.c_double: "double", ctypes.c_void_p: "pointer", ctypes.c_int: "int"}
    return {name: (restype_kind[res], [getattr(a, "kind", None) or native[a] for a in args])
            for name, (res, args) in table.items()}


def _prefix(name):
    return name[:name.index("_") + 1]


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_header_and_table_agree(header):
    """Per header the registry's rows against the prototypes, TYPE BY TYPE: the same names in the header's order, per function
    the return type and the number and kind of the parameters.  (A ctypes binding with a wrong argument type fails silently
    otherwise.)"""
    functions, _ = _parse_header(_read(header))
    table = _table_kinds(_lib.HEADERS[header])
    print(f"\n{header}: {len(functions)} entries")
    assert len(functions) == COUNTS[header]
    assert list(table) == list(functions)                                   # same names, in the header's order
    for name in functions:
        assert table[name] == functions[name], name
    if header == MAIN:
        assert sum(len(p) for _, p in functions.values()) > 400


def test_library_loads_and_exports_every_declared_symbol():
    """Registry, headers and the library's dynamic symbols name the same set, each entry in exactly one header and each header
    with a prefix of its own; the loaded library carries every row's types; per struct the fields in the header's order with
    the matching ctypes type; ABI version, struct sizes and build target."""
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(os.listdir(INCLUDE)) == sorted(_lib.HEADERS) == sorted(COUNTS)
    parsed = {header: _parse_header(_read(header)) for header in _lib.HEADERS}
    declared = [name for functions, _ in parsed.values() for name in functions]
    print(f"\n{len(declared)} entries over {len(parsed)} headers")
    assert len(declared) == len(set(declared)) == 72, sorted(n for n in set(declared) if declared.count(n) > 1)
    assert set(declared) == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == sum(len(t) for t in _lib.HEADERS.values())
    assert _lib.EXPORTED == list(_lib.SIGNATURES) == [name for table in _lib.HEADERS.values() for name in table]
    # one prefix per header, plain vgg_ for the main one, and no header's text (comments included) names another's
    prefixes = {header: {_prefix(name) for name in table} for header, table in _lib.HEADERS.items()}
    assert all(len(p) == 1 for p in prefixes.values()) and prefixes[MAIN] == {"vgg_"}
    assert len(set.union(*prefixes.values())) == len(prefixes)
    for header, (prefix,) in prefixes.items():
        for other in _lib.HEADERS:
            assert header in (MAIN, other) or prefix not in _read(other), (prefix, other)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert set(re.findall(r" T (vgg[a-z]?_\w+)$", nm, flags=re.M)) == set(_lib.SIGNATURES)
    functions, structs = parsed[MAIN]
    binding = {"vgg_ba_problem": _lib.BAProblem, "vgg_ba_options": _lib.BAOptions, "vgg_ba_iteration": _lib.BAIteration,
               "vgg_ba_summary": _lib.BASummary}
    assert set(structs) == set(binding) and not any(s for header, (_, s) in parsed.items() if header != MAIN)
    for name, st in binding.items():
        assert list(st._fields_) == structs[name], name
    assert len(structs["vgg_ba_problem"]) == 35
    for sym in _lib.SIGNATURES:
        assert hasattr(L, sym), sym
    L.vgg_build_arch.restype = ctypes.c_char_p
    assert L.vgg_build_arch() == b"gfx950"
    # the binding refuses a library with another struct layout: version and sizes are compared at load
    assert int(re.search(r"#define VGG_ABI_VERSION (\d+)", _read(MAIN)).group(1)) == _lib.ABI_VERSION == L.vgg_abi_version() == 2
    L.vgg_abi_sizeof.restype = ctypes.c_size_t
    assert [int(L.vgg_abi_sizeof(i)) for i in range(5)] == [ctypes.sizeof(t) for t in (_lib.BAProblem, _lib.BAOptions,
                                                                                       _lib.BAIteration, _lib.BASummary)] + [0]
    cov = _read("vggsfm_amd_covariance.h")
    assert tuple(int(re.search(rf"#define VGGC_COV_{k} (\d+)", cov).group(1)) for k in ("CAMERAS", "POINTS")) \
        == (_lib.COV_CAMERAS, _lib.COV_POINTS)
    loaded = _lib.lib()
    assert loaded.vgg_abi_version() == 2 == _lib.ABI_VERSION
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_one_copy_of_the_shared_host_state_of_the_ba_units():
    """The BA launches are spread over several translation units that share the tuning overrides, the profiler and the table
    of solves: among ALL symbols of the library, of any binding, each is defined exactly once.  (A `static` object in a shared
    header would give every unit a copy: vgg_ba_tuning would stop reaching the point and camera launchers while every
    numerical test still passed.)"""
    nm = subprocess.run(["nm", "--defined-only", "-C", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = [line.split(None, 2)[2] for line in nm.splitlines() if len(line.split(None, 2)) == 3]
    for name in ("vgg::g_tuning", "vgg::g_prof", "vgg::g_host_solves"):
        assert names.count(name) == 1, (name, names.count(name))


def test_the_header_parser_reads_kinds_and_field_order():
    """The comparison above is not vacuous: what the parser reads for a few declarations, pinned by hand (long / int /
    size_t told apart, parameter counts, field order), and a binding with cam_q / cam_t swapped -- same sizeof -- differs."""
    functions, structs = _parse_header(open(os.path.join(ROOT, "include", "vggsfm_amd.h")).read())
    assert functions["vgg_reproj_stats"] == ("int", ["pointer", "pointer", "long", "int", "pointer", "pointer", "size_t",
                                                     "pointer"])
    assert functions["vgg_depth_align"][1][10] == "unsigned long long" and functions["vgg_build_arch"] == ("pointer", [])
    assert functions["vgg_ba_tuning"] == ("int", ["int"] * 4) and functions["vgg_abi_sizeof"] == ("size_t", ["int"])
    names = [n for n, _ in structs["vgg_ba_problem"]]
    assert names.index("cam_q") + 1 == names.index("cam_t") and structs["vgg_ba_problem"][8] == ("loss_scale", ctypes.c_double)
    assert structs["vgg_ba_summary"][:3] == [("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                                             ("num_iterations", ctypes.c_int32)]
    swapped = list(_lib.BAProblem._fields_)
    q = names.index("cam_q")
    swapped[q], swapped[q + 1] = swapped[q + 1], swapped[q]
    assert swapped != structs["vgg_ba_problem"] and list(_lib.BAProblem._fields_) == structs["vgg_ba_problem"]
    wrong_row = list(functions["vgg_reproj_stats"][1])
    wrong_row[2], wrong_row[3] = wrong_row[3], wrong_row[2]
    assert wrong_row != [a.kind for a in _lib.SIGNATURES["vgg_reproj_stats"][1]]


def test_64_bit_values_reach_the_library():
    """Bare Python ints through the table: a long above 2^32 arrives whole (without argtypes ctypes passes a 32-bit int and
    both calls of a pair return the same size)."""
    L = _lib.lib()
    for fn in (L.vgg_reproj_stats_workspace_bytes, L.vgg_depth_align_workspace_bytes):
        small, big = fn(5), fn(2 ** 33 + 5)
        assert big != small and big > 2 ** 33, (small, big)


def test_out_of_range_arguments_are_refused_not_masked():
    """A value that does not fit its C type raises ctypes.ArgumentError before the library is entered (so the entries that
    need a GPU are safe to call here); bools, numpy integers and ctypes instances of the right type pass."""
    L = _lib.lib()
    with pytest.raises(ctypes.ArgumentError, match="does not fit the C type int"):
        L.vgg_cholesky_workspace_bytes(2 ** 31)
    try:
        with pytest.raises(ctypes.ArgumentError, match="does not fit the C type int"):
            L.vgg_ba_tuning(2 ** 32 + 8, 0, 0, 0)
    finally:
        assert L.vgg_ba_tuning(0, -1, 0, 0) == 0
    with pytest.raises(ctypes.ArgumentError, match="does not fit the C type size_t"):
        L.vgg_reproj_stats(None, None, 1, 0, None, None, -1, None)
    with pytest.raises(ctypes.ArgumentError):
        L.vgg_cholesky_workspace_bytes(1.5)
    with pytest.raises(ctypes.ArgumentError):
        L.vgg_cholesky_workspace_bytes(ctypes.c_double(3))
    want = L.vgg_cholesky_workspace_bytes(3)
    assert want > 0 and L.vgg_cholesky_workspace_bytes(True) == L.vgg_cholesky_workspace_bytes(1)
    for three in (np.int64(3), ctypes.c_int(3), ctypes.c_long(3)):
        assert L.vgg_cholesky_workspace_bytes(three) == want
