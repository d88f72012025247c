"""include/pmf_hip.h as data: every prototype and every struct, with each parameter's and field's exact C type.

Shared by the static checks of the two bindings (tests/test_julia_shim_static.py, tests/test_abi.py).  A type is spelled
canonically: single spaces, none around `*` ("const float*const*", "pmf_ctx**", "int64_t")."""
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "pmf_hip.h"

C_CLASS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "f32", "double": "f64", "uint64_t": "u64"}
C_SIZE = {"int": 4, "int32_t": 4, "int64_t": 8, "uint64_t": 8, "uint8_t": 1, "float": 4, "double": 8}


def _c_type(decl):
    """'const float *const *u0' -> 'const float*const*'; 'int64_t M' -> 'int64_t' (the declared name is dropped)."""
    m = re.fullmatch(r"(.*?)(\w+)", " ".join(decl.split()))
    assert m and m.group(1).strip(), decl
    return re.sub(r"\s*\*\s*", "*", m.group(1).strip())


def _class_of(ctype):
    """'const float*' -> 'ptr'; 'int64_t' -> 'i64'; a function-pointer typedef counts as a pointer."""
    if "*" in ctype or ctype == "pmf_host_allreduce_fn":
        return "ptr"
    assert ctype in C_CLASS, ctype
    return C_CLASS[ctype]


def _c_class(decl):
    """The same of a declaration: 'const float *w' -> 'ptr'; 'int64_t M' -> 'i64'."""
    return _class_of(_c_type(decl))


def parse():
    """-> (prototypes: name -> (return type, [parameter type, ...]), structs: name -> [(field, type), ...])."""
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const char \*)\s*(pmf_\w+)\s*\(([^()]*)\)\s*;", txt):
        params = params.strip()
        protos[name] = (ret.replace(" *", "*"), [] if params in ("", "void") else [_c_type(p) for p in params.split(",")])
    structs = {}
    for body, name in re.findall(r"typedef struct \w+\s*\{(.*?)\}\s*(\w+)\s*;", txt, flags=re.S):
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                first, *more = decl.split(",")                 # `int64_t n_rows, n_cols`: the further names share the type
                ctype = _c_type(first)
                fields += [(re.findall(r"\w+", d)[-1], ctype) for d in (first, *more)]
                assert not more or "*" not in decl, decl
        structs[name] = fields
    return protos, structs


def header():
    """The same by class of type (i32 / i64 / u64 / f32 / f64 / ptr): what the Julia shim is compared with."""
    protos, structs = parse()
    return ({n: ("ptr" if "*" in ret else "i32", [_class_of(t) for t in params]) for n, (ret, params) in protos.items()},
            {n: [(f, _class_of(t)) for f, t in fields] for n, fields in structs.items()})


def natural_size(fields):
    """sizeof a struct of these (field, type) pairs under natural alignment on an LP64 target."""
    off, align = 0, 1
    for _, t in fields:
        size = 8 if "*" in t else C_SIZE[t]
        off = -(-off // size) * size + size
        align = max(align, size)
    return -(-off // align) * align
