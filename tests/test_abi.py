"""The C-ABI shared library loads without a GPU and exports every symbol include/pmf_hip.h declares, and the ctypes
binding declares every function and every struct as the header does (_abi.SIGNATURES, _abi.STRUCTS)."""
import ctypes
import re
from pathlib import Path

import pytest

from abi_header import natural_size, parse

ROOT = Path(__file__).resolve().parent.parent
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double}


def ctypes_type(abi, ctype):
    """The one ctypes type for a C type of the header: `pmf_ctx *` and `void *` are c_void_p, `char *` is c_char_p, the
    function-pointer typedef is its CFUNCTYPE, a scalar or a struct is itself, and every further `*` is a POINTER()."""
    base, depth = re.sub(r"\bconst\b|\s|\*", "", ctype), ctype.count("*")
    if base == "pmf_host_allreduce_fn":
        t = abi.HOST_ALLREDUCE_FN
    elif base in ("void", "pmf_ctx", "char"):
        t, depth = (ctypes.c_char_p if base == "char" else ctypes.c_void_p), depth - 1
        assert depth >= 0, ctype
    elif base in abi.STRUCTS:
        t = abi.STRUCTS[base]
        assert depth >= 1, ctype                           # the header passes no struct by value
    else:
        t = SCALARS[base]
    for _ in range(depth):
        t = ctypes.POINTER(t)
    return t


def signature_errors(abi, signatures, protos):
    """Every way in which the table differs from the parsed prototypes, as text."""
    errs = [f"{n}: only in the {'table' if n in signatures else 'header'}" for n in sorted(set(signatures) ^ set(protos))]
    for name in sorted(set(signatures) & set(protos)):
        restype, argtypes = signatures[name]
        ret, params = protos[name]
        if restype is not ctypes_type(abi, ret):
            errs.append(f"{name}: returns {ret}, declared {restype}")
        if len(argtypes) != len(params):
            errs.append(f"{name}: takes {len(params)} parameters, {len(argtypes)} declared")
        for k, (got, c) in enumerate(zip(argtypes, params)):
            if got is not ctypes_type(abi, c):
                errs.append(f"{name}: parameter {k + 1} is {c}, declared {got}")
    return errs


def struct_errors(abi, mirrors, cstructs):
    errs = [f"{n}: only in the {'binding' if n in mirrors else 'header'}" for n in sorted(set(mirrors) ^ set(cstructs))]
    for name in sorted(set(mirrors) & set(cstructs)):
        got = [(f, t) for f, t, *_ in mirrors[name]._fields_]
        want = [(f, ctypes_type(abi, t)) for f, t in cstructs[name]]
        if got != want:
            errs.append(f"{name}: fields {got}, the header has {want}")
        if ctypes.sizeof(mirrors[name]) != natural_size(cstructs[name]):
            errs.append(f"{name}: sizeof {ctypes.sizeof(mirrors[name])}, the header's fields take {natural_size(cstructs[name])}")
    return errs


def declared_symbols():
    txt = (ROOT / "include" / "pmf_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pmf_[a-z_A-Z0-9]+)\s*\(", txt)))


def test_header_symbols_are_exported(pkg):
    syms = declared_symbols()
    assert len(syms) >= 40
    lib = ctypes.CDLL(str(ROOT / "pathmatfac.jl_amd" / "libpmf_hip.so"))
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/pmf_hip.h but not exported"
    assert sorted(pkg._lib.EXPORTS) == syms          # the ctypes binding covers exactly the header
    assert lib.pmf_version() == 1


def test_structs_match_header_layout(pkg):
    # pmf_fit_opts: 12 int32 + 2 double + 1 int64 ; pmf_fit_result: 4 int32 + double + pointer + double
    assert ctypes.sizeof(pkg._lib.FitOpts) == 12 * 4 + 2 * 8 + 8
    assert ctypes.sizeof(pkg._lib.FitResult) == 4 * 4 + 8 + 8 + 8


def test_missing_library_fails_loudly(pkg, tmp_path):
    import pytest
    with pytest.raises(pkg.PMFError):
        pkg._lib.load_library(tmp_path / "nope.so")


def test_plain_c_host_compiles_and_links(tmp_path):
    """examples/fit_c.c uses the boundary from C alone (no Python, no torch): it must compile against the header and
    link against the library (running it needs the GPU: tests/test_gpu_host.py)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        import pytest
        pytest.skip("gcc not available")
    exe = tmp_path / "fit_c"
    cmd = ["gcc", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "fit_c.c"),
           f"-L{ROOT / 'pathmatfac.jl_amd'}", "-lpmf_hip", f"-Wl,-rpath,{ROOT / 'pathmatfac.jl_amd'}", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert exe.exists()


# ---- the binding's signature table and struct mirrors against the header ---------------------------------------------------
def test_every_signature_matches_its_prototype(pkg):
    abi = pkg._abi
    protos, _ = parse()
    assert len(protos) == 91 and sorted(protos) == declared_symbols()
    assert protos["pmf_add_xreg_network"][1][5] == "const float*const*" and protos["pmf_last_error"] == ("const char*", [])
    assert set(abi.SIGNATURES) == set(protos) and pkg._lib.EXPORTS == list(abi.SIGNATURES)
    assert signature_errors(abi, abi.SIGNATURES, protos) == []
    lib = pkg._lib.load_library()
    by_path = pkg._lib.load_library(pkg._lib.LIB_PATH)      # a library loaded from an explicit path is declared too
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        for l in (lib, by_path):
            f = getattr(l, name)
            assert f.restype is restype and list(f.argtypes) == list(argtypes), name


def test_all_structs_mirror_the_header(pkg):
    abi = pkg._abi
    _, cstructs = parse()
    assert len(cstructs) == 8 and cstructs["pmf_csr"][:2] == [("n_rows", "int64_t"), ("n_cols", "int64_t")]
    assert struct_errors(abi, abi.STRUCTS, cstructs) == []
    for name in ("FitOpts", "FitResult", "LbfgsOpts", "LbfgsResult", "EmOpts", "EmResult", "SimOpts", "Csr"):
        assert getattr(pkg._lib, name) in abi.STRUCTS.values(), name


def test_the_check_rejects_what_it_is_there_to_find(pkg):
    abi = pkg._abi
    protos, cstructs = parse()
    P, S = ctypes.POINTER, abi.SIGNATURES

    def doctored(name, change):
        restype, argtypes = S[name]
        return {**S, name: (restype, change(list(argtypes)))}

    impute = S["pmf_impute"][1]
    assert impute[2] is ctypes.c_int64 and S["pmf_get_grad"][1][3] is P(ctypes.c_float)
    for bad, word in [
        (doctored("pmf_impute", lambda a: a[:2] + [ctypes.c_int] + a[3:]), "pmf_impute: parameter 3 is int64_t"),
        (doctored("pmf_get_grad", lambda a: a[:3] + [P(ctypes.c_double)]), "pmf_get_grad: parameter 4 is float*"),
        (doctored("pmf_set_lr", lambda a: a[:-1]), "pmf_set_lr: takes 2 parameters, 1 declared"),
    ]:
        errs = signature_errors(abi, bad, protos)
        assert len(errs) == 1 and word in errs[0], errs
    fields = list(abi.SimOpts._fields_)
    fields[0], fields[1] = fields[1], fields[0]
    swapped = type("SwappedSimOpts", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(swapped) == ctypes.sizeof(abi.SimOpts)
    errs = struct_errors(abi, {**abi.STRUCTS, "pmf_sim_opts": swapped}, cstructs)
    assert len(errs) == 1 and errs[0].startswith("pmf_sim_opts: fields"), errs


def test_a_wrong_argument_never_reaches_the_library(pkg):
    """ctypes refuses each of these while it converts the arguments, before the call: no GPU is touched."""
    lib = pkg._lib.load_library()
    with pytest.raises(ctypes.ArgumentError):
        lib.pmf_impute(None, 0, 1.5, 2, None, 1)                       # a float for an int64_t
    with pytest.raises(ctypes.ArgumentError):
        lib.pmf_set_lr(None, "0.1")                                    # a string for a float
    with pytest.raises(ctypes.ArgumentError):
        lib.pmf_get_grad(None, 0, 0, (ctypes.c_double * 4)())          # a double array for float *


def test_64_bit_values_cross_intact_as_plain_ints(pkg):
    """Nothing here sets argtypes or wraps a value: the installed table alone carries 64 bits."""
    lib = pkg._lib.load_library()
    off = ctypes.c_int64(0)
    assert lib.pmf_debug_impute_offset(199999, 49999, 200005, ctypes.byref(off)) == 0
    assert off.value == 49999 * 200005 + 199999 and off.value > 2 ** 32
