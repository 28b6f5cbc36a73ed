"""The Python binding — the ctypes signatures every test, tool and bench.py calls librt_amd.so through — checked mechanically against
include/rt_amd.h, as tests/test_rust_binding.py checks the Rust block: raytracinginrust_amd/_abi.py SIGNATURES must hold exactly the
header's functions, each with the header's arity and, argument by argument and for the return value, a ctypes type of the same class;
`CameraParams` must be rt_camera; the loaded libraries must carry the table's types; and nothing outside _abi.py may declare a header
function a second time.  The test also proves that it bites: copies of the table with one signature spoilt are reported."""
import ctypes as C
import os
import re

from conftest import ROOT
from raytracinginrust_amd import _abi
from raytracinginrust_amd._abi import SIGNATURES, CameraParams
from test_rust_binding import c_prototypes, camera_fields_c

# the header's scalar classes (test_rust_binding.C_SCALARS) -> the ctypes types that stand for them
SCALARS = {"i32": (C.c_int, C.c_int32), "u32": (C.c_uint32,), "u64": (C.c_uint64, C.c_ulonglong), "i64": (C.c_longlong, C.c_int64),
           "f64": (C.c_double,), "f32": (C.c_float,), "usize": (C.c_size_t,), "u8": (C.c_uint8,), "char": (C.c_char,)}
UNTYPED_POINTERS = (C.c_void_p, C.c_char_p)


def _header():
    return open(os.path.join(ROOT, "include", "rt_amd.h")).read()


def _pointee_ok(t, pointee):
    """Is ctypes type `t` what a pointer to the header's `pointee` may point at?"""
    if isinstance(pointee, tuple):                                  # a pointer to a pointer (double**, void**)
        return _matches(t, pointee)
    if pointee == "Camera":
        return t is CameraParams
    return t in SCALARS.get(pointee, ())                            # (void, rt_scene, rt_rng: opaque — c_void_p only)


def _matches(t, c_type):
    """Does ctypes type `t` stand for the header's type `c_type` (test_rust_binding._c_type's form)?"""
    kind, base = c_type
    if kind == "val":
        return t is None if base == "void" else t in SCALARS[base]
    if t in UNTYPED_POINTERS:
        return True
    return isinstance(t, type) and issubclass(t, C._Pointer) and _pointee_ok(t._type_, base)


def compare(table, protos, camera=CameraParams, header_camera=None):
    """Every disagreement between a signature table (name without prefix -> (restype, argtypes)) and the header's prototypes."""
    problems = []
    for name in sorted(set(protos) - {"rt_" + n for n in table}):
        problems.append(f"{name}: declared in include/rt_amd.h, missing from the table")
    for name, (res, args) in table.items():
        if "rt_" + name not in protos:
            problems.append(f"rt_{name}: not declared in include/rt_amd.h")
            continue
        cret, cargs = protos["rt_" + name]
        if cret[0] != "val" and res not in UNTYPED_POINTERS:
            problems.append(f"rt_{name}: returns a pointer ({cret}) but restype is {res}")
        elif cret[0] == "val" and not _matches(res, cret):
            problems.append(f"rt_{name}: restype {res} vs header {cret}")
        if len(args) != len(cargs):
            problems.append(f"rt_{name}: {len(args)} arguments vs header {len(cargs)}")
            continue
        for k, (a, c) in enumerate(zip(args, cargs)):
            if not _matches(a, c):
                problems.append(f"rt_{name}: argument {k} is {a} vs header {c}")
    if header_camera is not None:
        fields = [(n, getattr(t, "_length_", 1)) for n, t in camera._fields_]
        doubles = all((t._type_ if hasattr(t, "_length_") else t) is C.c_double for _, t in camera._fields_)
        if fields != header_camera or not doubles:
            problems.append(f"CameraParams fields {camera._fields_} vs rt_camera {header_camera}")
    return problems


def test_the_table_covers_the_header_and_agrees_with_it():
    hdr = _header()
    protos = c_prototypes(hdr)
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert set(protos) == declared and len(protos) >= 95                    # every prototype of the header was understood
    assert {"rt_" + n for n in SIGNATURES} == set(protos)                   # coverage, both directions
    assert compare(SIGNATURES, protos, header_camera=camera_fields_c(hdr)) == []
    assert SIGNATURES["device_count"][1] == [] and SIGNATURES["last_error"][1] == []
    assert set(_abi.BUILDER_NAMES) <= set(SIGNATURES)


def test_camera_params_is_rt_camera():
    want = camera_fields_c(_header())
    assert [(n, getattr(t, "_length_", 1)) for n, t in CameraParams._fields_] == want
    assert C.sizeof(CameraParams) == 8 * sum(k for _, k in want)

    class Swapped(C.Structure):
        _fields_ = [f for f in CameraParams._fields_ if f[0] != "vfov"] + [("vfov", C.c_double)]
    assert any("CameraParams" in p for p in compare(SIGNATURES, c_prototypes(_header()), camera=Swapped, header_camera=want))


def _carried(fn):
    return fn.restype, (None if fn.argtypes is None else list(fn.argtypes))


def test_the_loaded_libraries_carry_the_tables_types(pbe, obe):
    for name in c_prototypes(_header()):
        res, args = SIGNATURES[name[len("rt_"):]]
        assert _carried(getattr(pbe.lib, name)) == (res, list(args)), name
    for name in _abi.BUILDER_NAMES:
        res, args = SIGNATURES[name]
        assert _carried(getattr(obe.lib, "orc_" + name)) == (res, list(args)), name
        assert obe.fn(name) is getattr(obe.lib, "orc_" + name) and pbe.fn(name) is getattr(pbe.lib, "rt_" + name)


def test_a_library_that_lacks_symbols_is_an_error_that_names_them():
    class Fn:
        restype = argtypes = "unset"

    class Partial:
        _name = "partial.so"

    lib = Partial()
    for name in SIGNATURES:
        if name not in ("render_multi", "progressive_add"):
            setattr(lib, "rt_" + name, Fn())
    try:
        _abi.declare(lib, "rt_", SIGNATURES)
    except AttributeError as e:
        assert "rt_render_multi" in str(e) and "rt_progressive_add" in str(e) and "partial.so" in str(e)
    else:
        raise AssertionError("a partial library was accepted")
    _abi.declare(lib, "rt_", SIGNATURES, allow_missing=True)
    assert (lib.rt_render.restype, lib.rt_render.argtypes) == SIGNATURES["render"] and not hasattr(lib, "rt_render_multi")


def test_the_check_fails_on_a_spoilt_signature():
    protos = c_prototypes(_header())

    def reported(name, res, args):
        bad = dict(SIGNATURES)
        assert (res, args) != tuple(bad[name])
        bad[name] = (res, args)
        problems = compare(bad, protos)
        return problems != [] and all(p.startswith(f"rt_{name}:") for p in problems)

    res, args = SIGNATURES["moving_sphere"]
    assert reported("moving_sphere", res, args[:-2] + [args[-1], args[-2]])         # (.., radius, material) swapped
    res, args = SIGNATURES["render"]
    assert args[7] is C.c_uint64
    assert reported("render", res, args[:7] + [C.c_uint32] + args[8:])              # the seed as c_uint32
    res, args = SIGNATURES["rotate"]
    assert reported("rotate", res, args[:1] + args[2:])                             # one argument dropped
    assert SIGNATURES["scene_create"][0] is C.c_void_p
    assert reported("scene_create", C.c_int, [])                                    # restype never set: ctypes' default, a truncated pointer
    # and a function missing from the table, or one the header does not have
    assert any(p.startswith("rt_free:") for p in compare({k: v for k, v in SIGNATURES.items() if k != "free"}, protos))
    assert any(p.startswith("rt_no_such:") for p in compare({**SIGNATURES, "no_such": (C.c_int, [])}, protos))


ASSIGNMENT = re.compile(r"([\w\.\[\]\"']+?)\.(?:argtypes|restype)\b[^=\n]*=(?!=)")


def second_declarations(text, header_names):
    """Lines that assign `.argtypes` / `.restype` of a header function, or of something whose name cannot be read off the line."""
    found = []
    for k, line in enumerate(text.split("\n"), 1):
        for m in ASSIGNMENT.finditer(line):
            target = m.group(1).split(".")[-1]
            if target in header_names or not re.fullmatch(r"(rt|orc)_[a-z0-9_]+", target):
                found.append((k, line.strip()))
    return found


def test_no_header_function_is_declared_outside_the_table():
    names = set(c_prototypes(_header()))
    assert second_declarations("lib.rt_render.argtypes = [C.c_void_p]", names) and second_declarations("fn.restype, fn.argtypes = res, args", names)
    assert second_declarations("    be.lib.rt_free.restype = None; x = 1", names) and not second_declarations("lib.rt_debug_node_counts.restype = C.c_int", names)
    assert not second_declarations("assert fn.restype == C.c_int and lib.rt_render.argtypes is None", names)
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("raytracinginrust_amd", "tests", "tools"):
        for d, _, fs in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(d, f) for f in fs if f.endswith(".py")]
    assert len(files) > 60
    found = {}
    for path in files:
        if os.path.abspath(path) in (os.path.abspath(_abi.__file__), os.path.abspath(__file__)):
            continue
        hits = second_declarations(open(path).read(), names)
        if hits:
            found[os.path.relpath(path, ROOT)] = hits
    assert found == {}
