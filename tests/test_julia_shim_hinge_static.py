"""Static check of the squared-hinge noise models in julia/PathMatFacHIP.jl -- no Julia needed: the shim maps MatFac's
SquaredHingeNoise / OrdinalSqHingeNoise to the library's one kind 3, and `marshal!` holds one `ccall` of the literal
:pmf_set_noise_thresholds whose types match the prototype in include/pmf_hip.h (the parser is the one of
tests/test_julia_shim_static.py), sent after :pmf_set_noise, with the interior of ext_thresholds behind a -Inf."""
import re

import test_julia_shim_static as st

NAME = "pmf_set_noise_thresholds"


def _function(src, name):
    m = re.search(r"^function " + re.escape(name) + r"\(", src, flags=re.M)
    assert m, f"the shim does not define {name}"
    return src[m.start():src.index("\nend\n", m.start())]


def test_the_threshold_entry_is_bound_with_the_prototypes_types():
    protos, _ = st.header()
    assert protos[NAME] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr"])
    assert protos["pmf_get_noise_thresholds"] == ("i32", ["ptr", "ptr"])
    mine = [(line, parts) for line, parts in st.ccalls(st.SHIM.read_text()) if re.search(r":" + NAME + r"\b", parts[0])]
    assert len(mine) == 1, "one ccall of the literal :pmf_set_noise_thresholds"
    line, parts = mine[0]
    assert st.check_ccall(line, parts, protos) == NAME
    types = st.split_top(st.inner(parts[2]))
    assert types == ["Ptr{Cvoid}", "Cint", "Ptr{Int64}", "Ptr{Int64}", "Ptr{Cfloat}"]


def test_both_models_are_the_librarys_kind_three():
    src = st.strip_comments(st.SHIM.read_text())
    assert re.search(r'"bernoulli_sq_hinge" => Cint\(3\)', src) and re.search(r'"ordinal_sq_hinge3" => Cint\(3\)', src)
    hdr = st.HEADER.read_text()
    assert re.search(r"^#define PMF_NOISE_SQ_HINGE 3$", hdr, flags=re.M)
    # the struct names of simulate_params.jl:224-238, lower-cased without "Noise", map to the ABI's names
    assert '"squaredhinge" => "bernoulli_sq_hinge"' in src and '"ordinalsqhinge" => "ordinal_sq_hinge3"' in src
    assert "get(NOISE_STRUCT_NAMES, s, s)" in _function(st.SHIM.read_text(), "noise_name")


def test_marshal_sends_the_interior_thresholds_after_the_noise_model():
    src = st.SHIM.read_text()
    body = st.strip_comments(_function(src, "marshal!"))
    assert body.index(":pmf_set_noise,") < body.index(":pmf_set_noise_thresholds,") < body.index(":pmf_clear_xreg")
    assert "GC.@preserve hs he thr" in body
    th = st.strip_comments(_function(src, "hinge_thresholds"))
    assert "ext_thresholds[2:end-1]" in th and "Float32[-Inf, t[1], t[2]]" in th and "Float32[0, Inf, Inf]" in th
