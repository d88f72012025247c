"""Static check of simulate_data! in julia/PathMatFacHIP.jl -- no Julia needed: the ccalls of the literal :pmf_simulate_data
and :pmf_simulate_data_resident match the prototypes in include/pmf_hip.h (the parser is the one of
tests/test_julia_shim_static.py), the struct SimOpts mirrors pmf_sim_opts field by field, and `install!` re-points
PathMatFac.simulate_data!."""
import re

import test_julia_shim_static as st

NAME = "pmf_simulate_data"
PROTO = ("i32", ["ptr", "ptr", "i64", "i64", "ptr", "i64"])
FIELDS = [("seed", "u64"), ("row_offset", "i64"), ("noise", "f32"), ("frac_missing", "f32")]


def _function(src, name):
    m = re.search(r"^function " + re.escape(name) + r"\(", src, flags=re.M)
    assert m, f"the shim does not define {name}"
    return src[m.start():src.index("\nend\n", m.start())]


def _c_struct(name):
    txt = re.sub(r"/\*.*?\*/", "", st.HEADER.read_text(), flags=re.S)
    (body,) = re.findall(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", txt, flags=re.S)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    return [(re.findall(r"\w+", d)[-1], st._c_class(d)) for d in decls]


def test_the_three_entries_are_declared():
    protos, _ = st.header()
    assert protos[NAME] == PROTO and protos[NAME + "_device"] == PROTO
    assert protos[NAME + "_resident"] == ("i32", ["ptr", "ptr"])
    hdr = st.HEADER.read_text()
    assert "src/simulate_params.jl:219-251" in hdr and "Philox4x32-10" in hdr and "PMF_SIMULATE_CHUNK_ROWS" in hdr


def test_the_struct_mirrors_the_header():
    assert _c_struct("pmf_sim_opts") == FIELDS
    mine = st.jl_structs(st.SHIM.read_text())["SimOpts"]
    assert [f for f, _ in mine] == [f for f, _ in FIELDS]
    assert [st.jl_class(t) for _, t in mine] == [c for _, c in FIELDS]
    assert [t for _, t in mine] == ["UInt64", "Int64", "Cfloat", "Cfloat"]          # 24 bytes, no padding, as in C


def test_the_shim_binds_both_entries_with_the_prototypes_types():
    protos, _ = st.header()
    calls = st.ccalls(st.SHIM.read_text())
    host = [(line, parts) for line, parts in calls if re.search(r":" + NAME + r"\b", parts[0])]
    res = [(line, parts) for line, parts in calls if re.search(r":" + NAME + r"_resident\b", parts[0])]
    assert len(host) == 1 and len(res) == 1
    line, parts = host[0]
    assert st.check_ccall(line, parts, protos) == NAME
    assert st.split_top(st.inner(parts[2])) == ["Ptr{Cvoid}", "Ref{SimOpts}", "Int64", "Int64", "Ptr{Cfloat}", "Int64"]
    assert parts[3:] == ["ctx", "opts", "1", "M", "out", "M"]                        # every row, leading dimension M
    line, parts = res[0]
    assert st.check_ccall(line, parts, protos) == NAME + "_resident"
    assert st.split_top(st.inner(parts[2])) == ["Ptr{Cvoid}", "Ref{SimOpts}"]


def test_the_function_marshals_the_model_and_invalidates_the_device_copy():
    body = st.strip_comments(_function(st.SHIM.read_text(), "simulate_data!"))
    assert "model::PM.PathMatFacModel; noise=0.1" in body                          # the reference's keyword and default
    assert body.index("marshal!(ctx, model.matfac)") < body.index(":pmf_simulate_data_resident,") < body.index(":pmf_simulate_data,")
    assert "SimOpts(UInt64(seed), Int64(row_offset), Cfloat(noise), Cfloat(frac_missing))" in body
    assert "GC.@preserve out" in body and "model.data .= out" in body
    assert body.index("model.data .= out") < body.index("delete!(DATA_KEY, model)")


def test_install_repoints_it():
    body = st.strip_comments(st.SHIM.read_text())
    body = body[body.index("function install!"):]
    body = body[:body.index("\nend")]
    assert re.search(r"@eval PathMatFac simulate_data!\(model::PathMatFacModel; kwargs\.\.\.\) = "
                     r"Main\.PathMatFacHIP\.simulate_data!\(model; kwargs\.\.\.\)", body)
