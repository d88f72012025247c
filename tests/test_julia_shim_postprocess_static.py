"""Static check of the post-processing part of julia/PathMatFacHIP.jl against include/pmf_hip.h -- no Julia needed.  The new
`ccall`s (pmf_stage_whiten, pmf_stage_rotate_by_svd, pmf_stage_reorder_by_importance, pmf_stage_lambda_max) must match the
header's prototypes, and `install!` must re-point whiten!, rotate_by_svd!, reorder_by_importance! and the two reweight_eb!
methods.  The parsing helpers are those of tests/test_julia_shim_static.py."""
import re

import pytest

from test_julia_shim_static import SHIM, ccalls, check_ccall, header, strip_comments

NEW_ENTRIES = {"pmf_stage_whiten": ["ptr", "i64", "i32", "ptr", "ptr", "ptr", "ptr"],
               "pmf_stage_rotate_by_svd": ["ptr", "ptr", "ptr"],
               "pmf_stage_reorder_by_importance": ["ptr", "ptr"],
               "pmf_stage_lambda_max": ["ptr", "i32", "i32", "ptr", "ptr", "ptr"]}
INSTALLED = ["whiten!", "rotate_by_svd!", "reorder_by_importance!", "reweight_eb!"]


@pytest.fixture(scope="module")
def shim():
    return SHIM.read_text()


def test_the_header_declares_the_entries():
    protos, _ = header()
    for name, params in NEW_ENTRIES.items():
        assert protos[name] == ("i32", params), (name, protos.get(name))
    assert protos["pmf_gram"] == ("i32", ["ptr", "i32", "i32", "ptr", "ptr", "i32", "ptr"])


def test_the_new_ccalls_match_their_prototypes(shim):
    protos, _ = header()
    bound = [check_ccall(line, parts, protos) for line, parts in ccalls(shim)]
    for name in NEW_ENTRIES:
        assert name in bound, f"{name} is not bound in the shim"


def test_install_repoints_the_postprocessing_functions(shim):
    body = strip_comments(shim)
    body = body[body.index("function install!"):]
    body = body[:body.index("\nend")]
    for name in INSTALLED:
        assert re.search(r"@eval PathMatFac " + re.escape(name) + r"\(", body), f"install! does not @eval {name}"
        assert re.search(r"^function " + re.escape(name) + r"\(", shim, flags=re.M), f"the shim does not define {name}"
    for reg in ("L2Regularizer", "GroupRegularizer"):                       # both reweight_eb! methods, by their first argument
        assert re.search(r"@eval PathMatFac reweight_eb!\(reg::" + reg + r", X::AbstractMatrix; kwargs\.\.\.\)", body), reg
        assert re.search(r"^function reweight_eb!\(\w+::PM\." + reg + r", X::AbstractMatrix;", shim, flags=re.M), reg
    # the permutation the library returns is 0-based: the shim adds 1 before it indexes Julia arrays with it
    reorder = shim[shim.index("function reorder_by_importance!"):]
    reorder = reorder[:reorder.index("\nend")]
    assert "Int.(perm) .+ 1" in reorder and reorder.count("PM.reorder_reg!") == 2
