"""TEST INFRASTRUCTURE: what every tests/test_*_abi.py checks of include/sdm.h against the binding, stated once.  The
literals - sizes, argument counts, offsets, flag values, byte formulas - stay in the tests: they are the assertions."""
import ctypes as C
import os
import re

from semantic_dsp_map_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sdm.h")).read()


def declared_functions(header="sdm.h"):
    """the sdm_* functions a header of include/ declares, sorted"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sdm_[a-z0-9_]+)\s*\(", text)))


def struct_fields(name):
    """the field names of `typedef struct { ... } name;` in declaration order"""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [re.sub(r"\[\d+\]", "", first.split()[-1])] + [re.sub(r"\[\d+\]", "", r.strip()) for r in rest]
    return tuple(fields)


def define(name):
    """the integer value of `#define name value` in the header"""
    return int(re.search(r"#define\s+%s\s+(\w+)" % name, HEADER).group(1).rstrip("u"), 0)


def assert_bound(n_args):
    """n_args: {function: k} - each is declared in the header, exported by the library and bound with k arguments"""
    names = declared_functions()
    lib = C.CDLL(binding.LIB_PATH)
    L = binding.load_library()
    for n, k in n_args.items():
        assert n in names and hasattr(lib, n) and getattr(L, n).argtypes is not None, n
        assert len(getattr(L, n).argtypes) == k, n
    return L


def alignment(dt):
    """of a field's type: its base type's, and for a nested struct the largest of its leaves'"""
    base = dt.base
    return base.alignment if base.names is None else max(alignment(base.fields[f][0]) for f in base.names)


def assert_layout(dtype, c_name, size):
    """dtype is the header's struct c_name: the size, the field names in the header's order, the header's `/* N bytes`
    comment, no hidden padding (the offsets are the running sum of the sizes) and every field naturally aligned"""
    assert dtype.itemsize == size, c_name
    assert dtype.names == struct_fields(c_name), c_name
    assert re.search(r"typedef struct \{\s*/\* %d bytes(?: \*/|[:,])[^}]*\}\s*%s;" % (size, c_name), HEADER), c_name
    at = 0
    for f in dtype.names:
        assert dtype.fields[f][1] == at, (c_name, f)
        assert at % alignment(dtype.fields[f][0]) == 0, (c_name, f)
        at += dtype.fields[f][0].itemsize
    assert at == dtype.itemsize, c_name
