"""The one gate over the components of the library's C ABI, CPU only.  A component is a public header, a source directory, one entry of
satools_amd._lib.COMPONENTS and (where its GPU tests are table-driven) a bounds table; "core" is include/satools_hip.h with csrc/*.hip.
Held against each other here, for every component alike: the component names, the entry-point names in both directions, every argument's
and result's kind, the five descriptor mirrors field by field, one header per name, the ABI number, the error a stale library gets, what
the build compiles, and the coverage of the bounds tables.  What is particular to one component (its constants, its ops, the conditions
on its own rows) stays in that component's host test."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

import abi_decl
from satools_amd import _lib, build
from satools_amd import f0 as f0_hip

ROOT = abi_decl.ROOT
CSRC = os.path.join(ROOT, "sa-toolkit_amd", "csrc")
NAMES = list(_lib.COMPONENTS)

# the sorted entry list of every component but the core, literally
ENTRIES = {
    "stats": ["sat_eer_bootstrap_i32"],
    "conv2d16": ["sat_conv2d_f16x3_f32"],
    "ragged": ["sat_attentive_stats_segments_f32", "sat_instnorm_segments_f32", "sat_melspec_logmel_segments_f32", "sat_res2_chain_segments_f32",
               "sat_row_mean_segments_f32", "sat_se_gate_add_segments_f32"],
    "ragged2d": ["sat_conv2d_segments_f32", "sat_plane_mean_segments_f32", "sat_row_mean_std_segments_f32", "sat_se_scale_add_relu_segments_f32"],
    "ragged2d16": ["sat_conv2d_f16x3_segments_f32"],
    "yaapt_long": ["sat_yaapt_long_f32", "sat_yaapt_long_workspace_bytes"],
    "geninput": ["sat_generator_input_f32"],
}
# descriptor struct -> (component that declares it, its ctypes mirror)
MIRRORS = {
    "sat_conv1d_desc": ("core", _lib.ConvDesc),
    "sat_tdnnf_layer_desc": ("core", _lib.TdnnfLayerDesc),
    "sat_mrf_desc": ("core", _lib.MrfDesc),
    "sat_yaapt_plan": ("core", f0_hip.YaaptPlan),
    "sat_geninput_desc": ("geninput", _lib.GenInputDesc),
}
# source files the build must find, where a component's name does not say it
SOURCES = {"ragged2d16": ["conv2d_f16x3_segments.hip"], "yaapt_long": ["yaapt_long.hip"], "geninput": ["generator_input.hip"]}
# component -> the GPU test module whose ROWS / FAMILIES table covers its entry points and kernel families
BOUNDS = {
    "core": "test_hip_bounds",
    "stats": "test_hip_eer_bootstrap",
    "conv2d16": "test_hip_conv2d16",
    "ragged": "test_hip_xvector_ragged",
    "ragged2d": "test_hip_xvector_resnet_ragged",
    "ragged2d16": "test_hip_xvector_resnet_ragged16",
    "yaapt_long": None,         # no table: tests/test_hip_yaapt_long.py calls moat directly, case by case
    "geninput": None,           # no table: tests/test_hip_geninput.py calls moat directly, case by case
}
# words the core header has never carried (a component is added WITHOUT touching it), besides every component's header and entry names
CORE_HEADER_SILENT_ON = ("eer_bootstrap", "f16x3_f32", "conv2d16", "ragged2d16", "yaapt_long", "generator_input", "geninput")


def _directory(component):
    return CSRC if component == "core" else os.path.join(CSRC, component)


def _sources(component):
    return [s for s in build.sources() if os.path.dirname(s) == _directory(component)]


# ---- 1: the names --------------------------------------------------------------------------------------------------------------------
def test_bindings_directories_and_headers_name_the_same_components():
    assert NAMES[0] == "core" and set(ENTRIES) == set(BOUNDS) - {"core"} == set(NAMES) - {"core"}
    assert set(NAMES) - {"core"} == set(build.components())                       # a directory with a .hip file <-> a binding
    found = {re.fullmatch(r"satools_hip_(\w+)\.h", f).group(1) for f in os.listdir(abi_decl.INCLUDE) if f != "satools_hip.h"}
    assert set(NAMES) - {"core"} == found                                         # a public header <-> a binding
    assert [_lib.header(c) for c in NAMES] == ["satools_hip.h"] + [f"satools_hip_{c}.h" for c in NAMES[1:]]
    with pytest.raises(KeyError):
        _lib.header("no_such_component")
    assert _lib.symbols() == sorted(n for c in NAMES for n in _lib.symbols(c)) and len(_lib.symbols()) == len(set(_lib.symbols())) >= 96


# ---- 2: header <-> binding <-> library, by name ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", NAMES)
def test_header_binding_and_library_hold_the_same_names(component):
    declared = abi_decl.names(_lib.header(component))
    assert declared == _lib.symbols(component) == sorted(_lib.COMPONENTS[component]) and len(declared) == len(set(declared))
    assert "sat_status" not in declared                                           # (the enum's typedef is no entry point)
    if component == "core":
        assert len(declared) >= 80 and "sat_conv1d_f32" in declared and "sat_row_mean_std_f32" in declared
    else:
        assert declared == ENTRIES[component]
    lib = _lib.lib()
    for n in declared:
        fn = getattr(lib, n)
        res, args = _lib.COMPONENTS[component][n]
        assert fn.restype is res and fn.argtypes is not None and list(fn.argtypes) == list(args), n


# ---- 3: every argument's kind -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", NAMES)
def test_every_argument_and_result_has_the_headers_kind(component):
    protos = _lib.COMPONENTS[component]
    for name, ret, kinds in abi_decl.entry_points(_lib.header(component)):
        res, args = protos[name]
        assert abi_decl.ctypes_agrees(ret, res), (name, ret, res)
        assert len(kinds) == len(args), (name, kinds, args)
        for i, (kind, ctype) in enumerate(zip(kinds, args)):
            assert abi_decl.ctypes_agrees(kind, ctype), (name, i, kind, ctype)


def test_the_kind_map_tells_the_types_apart():
    """the comparison of check 3 can fail: widths, signs, floats and pointers are distinct kinds; int / int32_t are one machine type"""
    ok = abi_decl.ctypes_agrees
    assert ok("int", C.c_int) and ok("int", C.c_int32) and ok("int64_t", C.c_int64) and ok("long long", C.c_int64) and ok("size_t", C.c_size_t)
    assert not ok("int64_t", C.c_int) and not ok("int", C.c_int64) and not ok("uint32_t", C.c_int) and not ok("float", C.c_int) and not ok("int", C.c_float)
    assert not ok("size_t", C.c_int64) and not ok("void", C.c_int) and ok("void", None) and not ok("int", None)
    assert ok("float*", C.c_void_p) and ok("sat_mrf_desc*", C.POINTER(_lib.MrfDesc)) and ok("int32_t*", C.POINTER(C.c_int32)) and ok("float**", C.POINTER(C.c_void_p))
    assert not ok("float*", C.c_int64) and not ok("int", C.c_void_p) and not ok("float*", C.c_char_p) and not ok("float", C.c_void_p)
    assert ok("char*", C.c_char_p) and not ok("char*", C.c_void_p)
    assert ok("float", C.c_float * 6, [6]) and not ok("float", C.c_float * 6, [5]) and not ok("float", C.c_float * 6) and not ok("float", C.c_float, [6])
    assert ok("void*", ((C.c_void_p * 2) * 3) * 4, [4, 3, 2]) and not ok("void*", ((C.c_void_p * 2) * 3) * 4, [2, 3, 4])


# ---- 4: the descriptor mirrors ------------------------------------------------------------------------------------------------------------
def test_every_struct_of_the_headers_has_a_mirror_and_no_other():
    found = {name: c for c in NAMES for name in abi_decl.structs(_lib.header(c))}
    assert found == {name: c for name, (c, _) in MIRRORS.items()}


@pytest.mark.parametrize("struct", list(MIRRORS))
def test_mirror_agrees_with_its_struct_field_by_field(struct):
    component, mirror = MIRRORS[struct]
    fields = abi_decl.structs(_lib.header(component))[struct]
    assert fields and [f for f, _, _ in fields] == [f for f, _ in mirror._fields_]  # names, in order
    for (field, kind, dims), (_, ctype) in zip(fields, mirror._fields_):
        assert abi_decl.ctypes_agrees(kind, ctype, dims), (struct, field, kind, dims, ctype)
    assert struct in mirror.__doc__
    if struct == "sat_geninput_desc":
        assert C.sizeof(mirror) == 10 * 4 + 3 * 8 + 8 * 8


# ---- 5: one header per name -----------------------------------------------------------------------------------------------------------------
def test_every_name_is_declared_in_exactly_one_header():
    declared = {c: set(abi_decl.names(_lib.header(c))) for c in NAMES}
    for a in NAMES:
        for b in NAMES:
            if a != b:
                assert not declared[a] & declared[b], (a, b)
                code = abi_decl.code(_lib.header(b))                              # nor otherwise mentioned in another header's code
                assert not [n for n in declared[a] if re.search(r"\b" + n + r"\b", code)], (a, b)
    core = open(os.path.join(abi_decl.INCLUDE, "satools_hip.h")).read()          # comments included
    assert "satools_hip_" not in core and not [w for w in CORE_HEADER_SILENT_ON if w in core]
    assert not [n for c in NAMES[1:] for n in declared[c] if n in core]


# ---- 6: the ABI number ------------------------------------------------------------------------------------------------------------------------
def test_abi_version_of_header_and_library():
    assert int(abi_decl.define("satools_hip.h", "SAT_ABI_VERSION")) == _lib.lib().sat_abi_version() == 8
    for c in NAMES[1:]:                                                           # entries are added without a new number: one define, in the core
        assert "SAT_ABI_VERSION" not in abi_decl.code(_lib.header(c)) and "define SAT_ABI_VERSION" not in open(os.path.join(abi_decl.INCLUDE, _lib.header(c))).read()


# ---- 7: a stale library ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", NAMES)
def test_a_library_without_an_entry_is_reported_with_the_build_command(component, monkeypatch):
    """what a library built before an entry existed looks like to the binding: a name of the table that dlsym cannot find"""
    name = f"sat_{component}_entry_of_a_newer_tree_f32"
    monkeypatch.setitem(_lib.COMPONENTS[component], name, (C.c_int, []))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.SatError, match=rf"does not export {name}.*older source tree.*build\.py"):
        _lib.lib()


# ---- 8: the build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", NAMES)
def test_build_compiles_the_components_directory_and_depends_on_its_header(component):
    src = _sources(component)
    assert src and all(s.endswith(".hip") for s in src) and src == sorted(src)
    assert [os.path.basename(s) for s in src] == SOURCES.get(component, [os.path.basename(s) for s in src])
    for s in src:
        base = os.path.basename(s)
        assert build.object_name(s) == (base + ".o" if component == "core" else f"{component}_{base}.o")
    headers = [os.path.normpath(h) for h in build.headers()]
    assert all(os.path.exists(h) for h in headers) and len(headers) == len(set(headers))
    assert os.path.join(abi_decl.INCLUDE, _lib.header(component)) in headers
    for f in os.listdir(_directory(component)):                                   # and on every header next to the sources
        if f.endswith(".h"):
            assert os.path.join(_directory(component), f) in headers, f


def test_build_lists_every_source_once_under_a_name_of_its_own():
    src = build.sources()
    assert sorted(src) == sorted(s for c in NAMES for s in _sources(c)) and len(src) == len(set(src))
    assert len({build.object_name(s) for s in src}) == len(src)
    assert src[:len(_sources("core"))] == _sources("core")                        # the core first, then the components in sorted order
    assert [os.path.basename(os.path.dirname(s)) for s in src[len(_sources("core")):]] == sorted(os.path.basename(os.path.dirname(s)) for s in src[len(_sources("core")):])
    assert build.object_name(os.path.join(CSRC, "x.hip")) == "x.hip.o" and build.object_name(os.path.join(CSRC, "stats", "x.hip")) == "stats_x.hip.o"


# ---- 9, 10: the coverage of the bounds tables -------------------------------------------------------------------------------------------------
def _launch_check_names(directory):
    """the kernel family names the sources of one directory hand to SAT_LAUNCH_CHECK"""
    names = set()
    for f in sorted(os.listdir(directory)):
        if f.endswith((".hip", ".h")):
            for args in re.findall(r"SAT_LAUNCH_CHECK\(([^;]*)\);", open(os.path.join(directory, f)).read()):
                names.update(re.findall(r'"([^"]+)"', args))
    return names


@pytest.mark.parametrize("component", [c for c in NAMES if BOUNDS[c]])
def test_every_entry_point_has_a_bounds_row(component):
    hb = importlib.import_module(BOUNDS[component])
    assert not torch.cuda.is_initialized()          # importing the table touches no GPU
    names = abi_decl.names(_lib.header(component))
    rows = {r.entry for r in hb.ROWS}
    exempt = getattr(hb, "EXEMPT", {})
    assert names and (component == "core" or not exempt)
    for n, why in exempt.items():                   # the core alone: an entry that launches no kernel has nothing to bound
        assert n in names, f"{n} is exempt but not in the header"
        assert n not in rows, f"{n} is exempt and has a row"
        assert why.startswith("launches no kernel") or (n == "sat_clock_probe" and why.startswith("diagnostic")), (n, why)
    missing = [n for n in names if n not in rows and n not in exempt]
    assert not missing, f"entry points without a bounds row: {missing}"
    assert not [r for r in rows if r not in names]
    for r in hb.ROWS:
        assert r.shapes, r.name


@pytest.mark.parametrize("component", [c for c in NAMES if BOUNDS[c]])
def test_the_dispatch_family_list_is_the_one_in_the_sources(component):
    """FAMILIES (+ INNER) of the bounds table = the SAT_LAUNCH_CHECK strings of the component's directory (the diagnostic clock probe aside):
    a new kernel family without a row that reaches it fails here, before it fails on the GPU"""
    hb = importlib.import_module(BOUNDS[component])
    names = _launch_check_names(_directory(component)) - {"clock_probe_kernel"}
    inner = getattr(hb, "INNER", {})
    assert names and (component != "core" or len(names) > 60)
    listed = set(hb.FAMILIES) | set(inner)
    assert listed == names, (sorted(names - listed), sorted(listed - names))
    assert len(hb.FAMILIES) == len(set(hb.FAMILIES)) and not set(hb.FAMILIES) & set(inner)
    assert set(inner.values()) <= {r.entry for r in hb.ROWS}


def test_components_without_a_table_are_the_two_whose_gpu_tests_call_moat_directly():
    assert [c for c in NAMES if BOUNDS[c] is None] == ["yaapt_long", "geninput"]
    for c, module in (("yaapt_long", "test_hip_yaapt_long.py"), ("geninput", "test_hip_geninput.py")):
        text = open(os.path.join(ROOT, "tests", module)).read()
        assert "moat" in text and not re.search(r"^(ROWS|FAMILIES) =", text, flags=re.M), module
        assert [n for n in ENTRIES[c] if n in text], module
