"""not gpu: the binding's prototype table (gr_amps_amd/capi.py: PROTOTYPES) against the declarations of include/amps_recc.h, and what
load() does with a library that lacks some of the table's entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import textwrap

import pytest

from gr_amps_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
RETURNS = {"int": C.c_int, "uint32_t": C.c_uint32, "size_t": C.c_size_t, "void": None, "const char *": C.c_char_p}


def _declarations():
    """[(return type, name, [parameter, ...])] of the header, comments stripped, parameter lists over several lines included"""
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    found = re.findall(r"^[ \t]*([A-Za-z_][\w \t]*?[ \t\*]+)(amps_(?:recc|bch)_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M)
    out = []
    for ret, name, params in found:
        params = " ".join(params.split())
        out.append((" ".join(ret.split()), name, [] if params in ("", "void") else [p.strip() for p in params.split(",")]))
    return out


def _is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_the_parser_finds_every_declaration():
    """guards the test below: every amps_recc_ / amps_bch_ name that is followed by a parenthesis in the header's code is a parsed
    declaration, once"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "amps_recc.h")).read(), flags=re.S)
    names = [d[1] for d in _declarations()]
    assert len(names) == len(set(names)) == 68
    assert set(names) == set(re.findall(r"\b(amps_(?:recc|bch)_[a-z_0-9]+)\s*\(", hdr))


def test_the_table_is_the_header():
    decls = _declarations()
    assert [d[1] for d in decls] == list(capi.PROTOTYPES) == list(capi.EXPORTS)        # every name, no other, in the header's order
    assert isinstance(capi.EXPORTS, tuple)
    for ret, name, params in decls:
        restype, argtypes = capi.PROTOTYPES[name]
        assert restype is RETURNS[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            if "*" in p or "[" in p:
                assert _is_pointer(t), (name, p, t)
            else:
                assert t is SCALARS[re.sub(r"\bconst\b", "", p).split()[0]], (name, p, t)
    assert capi.PROTOTYPES["amps_recc_debug_exact_slice"][1] == [C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]


def test_the_loaded_library_carries_the_table():
    L = capi.load()
    for name, (restype, argtypes) in capi.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name


CHILD = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, sys.argv[1])
    from gr_amps_amd import capi
    if not os.environ.get("AMPS_RECC_LIB"):
        capi.LIB_PATH = sys.argv[2]                 # the same file in the place of the tree's own library
    assert capi.LIB_PATH == sys.argv[2]
    try:
        capi.load()
        print("LOADED")
    except (ImportError, AttributeError) as e:
        print(type(e).__name__, e)
""")


@pytest.fixture(scope="module")
def tiny_library(tmp_path_factory):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler (cc, gcc, clang) to build a library with one export")
    d = tmp_path_factory.mktemp("tiny")
    src, lib = d / "tiny.c", d / "libtiny.so"
    src.write_text("int amps_recc_abi_version(void) { return 4; }\n")
    subprocess.run([cc, "-shared", "-fPIC", "-o", str(lib), str(src)], check=True)
    return str(lib)


def _child(lib, env_lib):
    env = {k: v for k, v in os.environ.items() if k != "AMPS_RECC_LIB"}
    if env_lib:
        env["AMPS_RECC_LIB"] = lib
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, lib], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.strip()


def test_an_ab_library_may_lack_entry_points(tiny_library):
    """AMPS_RECC_LIB names a library of another revision: load() gets past the prototype loop, and the first entry point it calls
    that the library lacks (the amps_recc_burst_size self-check) is the AttributeError ctypes gives for a missing symbol"""
    out = _child(tiny_library, env_lib=True)
    assert out.startswith("AttributeError") and "amps_recc_burst_size" in out, out


def test_the_trees_own_library_may_not(tiny_library):
    """without AMPS_RECC_LIB the same file is an ImportError that names what is missing: all of the table but the one export"""
    out = _child(tiny_library, env_lib=False)
    assert out.startswith("ImportError"), out
    for name in capi.EXPORTS:
        assert (name in out) == (name != "amps_recc_abi_version"), name
