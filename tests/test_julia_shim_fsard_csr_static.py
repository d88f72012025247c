"""Static check of the sparse update_A! entry in julia/PathMatFacHIP.jl -- no Julia needed: the shim holds a `ccall` of the
literal :pmf_fsard_update_A_csr whose types match the prototype in include/pmf_hip.h (the parser is the one of
tests/test_julia_shim_static.py), the CSR it hands over is the 0-based colptr / rowval of the transposed SparseMatrixCSC,
and the update_A! twin references both entries and chooses by L * K at the dense entry's capacity, as update_A_ does."""
import re

import fsard_ref as fr
import test_julia_shim_static as st

NAME = "pmf_fsard_update_A_csr"


def _calls():
    return st.ccalls(st.SHIM.read_text())


def _function(src, name):
    """The text of `function name(...) ... end` at the top level of the module."""
    m = re.search(r"^function " + re.escape(name) + r"\(", src, flags=re.M)
    assert m, f"the shim does not define {name}"
    return src[m.start():src.index("\nend\n", m.start())]


def test_the_sparse_entry_is_bound_with_the_prototypes_types():
    protos, _ = st.header()
    assert protos[NAME] == ("i32", ["ptr", "i64", "i64", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "f32", "f32", "f32", "ptr",
                                    "ptr", "i32", "i32", "f64", "ptr", "ptr", "ptr"])
    dense = protos["pmf_fsard_update_A"][1]
    assert protos[NAME][1] == dense[:4] + ["ptr", "ptr", "ptr"] + dense[5:]      # only `const float *S` changes
    mine = [(line, parts) for line, parts in _calls() if re.search(r":" + NAME + r"\b", parts[0])]
    assert len(mine) == 1, "one ccall of the literal :pmf_fsard_update_A_csr"
    line, parts = mine[0]
    assert st.check_ccall(line, parts, protos) == NAME
    types = st.split_top(st.inner(parts[2]))
    assert types[4:7] == ["Ptr{Int64}", "Ptr{Int32}", "Ptr{Cfloat}"]              # rowptr, col, val: the element widths too


def test_the_csr_is_the_zero_based_transposed_csc():
    body = st.strip_comments(_function(st.SHIM.read_text(), "fsard_update_A_csr!"))
    assert re.search(r"colptr \.- 1", body) and re.search(r"rowval \.- 1", body) and "nzval" in body
    assert "GC.@preserve rowptr col val" in body


def test_the_update_A_twin_references_both_entries_and_routes_by_capacity():
    src = st.SHIM.read_text()
    body = st.strip_comments(_function(src, "update_A!"))
    assert "fsard_update_A_csr!(" in body and re.search(r"\bfsard_update_A!\(", body)
    assert "SparseMatrixCSC(transpose(reg.S[v]))" in body
    assert re.search(r"L \* K > FSARD_DENSE_CAPACITY", body)
    m = re.search(r"^const FSARD_DENSE_CAPACITY = (\d+)", src, flags=re.M)
    assert m and int(m.group(1)) == fr.CAPACITY
    assert all(f":{k}" in body for k in ("auto", "dense", "sparse"))
