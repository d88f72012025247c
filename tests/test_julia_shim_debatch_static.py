"""Static check of remove_batch_effect in julia/PathMatFacHIP.jl -- no Julia needed: one `ccall` of the literal
:pmf_remove_batch_effect whose types match the prototype in include/pmf_hip.h (the parser is the one of
tests/test_julia_shim_static.py), the flag bits of the header, and `install!` re-pointing PathMatFac.remove_batch_effect."""
import re

import test_julia_shim_static as st

NAME = "pmf_remove_batch_effect"
PROTO = ("i32", ["ptr", "i32", "i64", "i64", "ptr", "i64", "ptr", "i64"])


def _function(src, name):
    m = re.search(r"^function " + re.escape(name) + r"\(", src, flags=re.M)
    assert m, f"the shim does not define {name}"
    return src[m.start():src.index("\nend\n", m.start())]


def test_the_three_entries_are_declared():
    protos, _ = st.header()
    assert protos[NAME] == PROTO and protos[NAME + "_device"] == PROTO
    assert protos[NAME + "_entries"] == ("i32", ["ptr", "i32", "i64", "ptr", "ptr", "ptr", "ptr"])
    hdr = st.HEADER.read_text()
    assert re.search(r"^#define PMF_DEBATCH_LINK 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PMF_DEBATCH_FILL_MISSING 2\b", hdr, flags=re.M)
    assert "src/remove_batch_effect.jl:3-16" in hdr and "src/layers.jl:240-253" in hdr


def test_the_shim_binds_the_host_entry_with_the_prototypes_types():
    protos, _ = st.header()
    mine = [(line, parts) for line, parts in st.ccalls(st.SHIM.read_text()) if re.search(r":" + NAME + r"\b", parts[0])]
    assert len(mine) == 1, "one ccall of the literal :pmf_remove_batch_effect"
    line, parts = mine[0]
    assert st.check_ccall(line, parts, protos) == NAME
    types = st.split_top(st.inner(parts[2]))
    assert types == ["Ptr{Cvoid}", "Cint", "Int64", "Int64", "Ptr{Cfloat}", "Int64", "Ptr{Cfloat}", "Int64"]
    args = parts[3:]
    assert args[2:4] == ["rows.start", "rows.stop"] and args[5] == args[7] == "length(rows)"   # Z holds exactly the rows asked for


def test_the_function_marshals_the_model_and_keeps_its_arrays_alive():
    body = st.strip_comments(_function(st.SHIM.read_text(), "remove_batch_effect"))
    assert "model::PM.PathMatFacModel, Z::AbstractMatrix" in body
    assert body.index("marshal!(ctx, model.matfac)") < body.index(":pmf_remove_batch_effect,")
    assert "GC.@preserve Z32 out" in body and "Z32 = f32(Z)" in body
    assert "(link ? 1 : 0) | (fill_missing ? 2 : 0)" in body


def test_install_repoints_it():
    body = st.strip_comments(st.SHIM.read_text())
    body = body[body.index("function install!"):]
    body = body[:body.index("\nend")]
    assert re.search(r"@eval PathMatFac remove_batch_effect\(model::PathMatFacModel, Z::AbstractMatrix; kwargs\.\.\.\) = "
                     r"Main\.PathMatFacHIP\.remove_batch_effect\(model, Z; kwargs\.\.\.\)", body)
