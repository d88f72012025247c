"""Static check of julia/PathMatFacHIP.jl against include/pmf_hip.h -- no Julia needed.

A small balanced-parenthesis scan finds every `ccall(` of the shim and compares it with the C prototype: the function name
must be a literal `:pmf_*` symbol the header declares (only the library part of the target may be computed), the return type
`Cint` (`Cstring` for pmf_last_error), the type tuple as long as the prototype's parameter list and as the argument list,
and every type of the right class.  The Julia mirrors of the header's structs must have its field order and types.
`install!` must re-point every function the shim replaces, and every entry the hosts need must be bound.
What this cannot see: run-time behaviour -- array shapes and layouts handed to the pointers, GC.@preserve coverage, the
PathMatFac / MatFac / Flux names the shim refers to.  The file is not executed here."""
import re
from pathlib import Path

import pytest

from abi_header import HEADER, _c_class, header  # noqa: F401  (the other shim checks read these through this module)

ROOT = Path(__file__).resolve().parent.parent
SHIM = ROOT / "pathmatfac.jl_amd" / "julia" / "PathMatFacHIP.jl"

JL_CLASS = {"Cint": "i32", "Int64": "i64", "Cfloat": "f32", "Cdouble": "f64", "UInt64": "u64", "Cstring": "ptr"}
STRUCTS = {"FitOpts": "pmf_fit_opts", "FitResult": "pmf_fit_result", "LbfgsOpts": "pmf_lbfgs_opts",
           "LbfgsResult": "pmf_lbfgs_result", "EmOpts": "pmf_em_opts", "EmResult": "pmf_em_result"}
INSTALLED = ["mf_fit!", "init_mu!", "init_logsigma!", "reweight_col_losses!", "construct_minimal_regularizer",
             "theta_delta_em", "update_A!"]
BOUND = ["pmf_stats", "pmf_get_precision", "pmf_comm_info", "pmf_reset_optimizer_state", "pmf_get_noise_weights",
         "pmf_stage_init_logsigma", "pmf_stage_reweight_col_losses", "pmf_stage_minimal_group_weights",
         "pmf_stage_theta_delta_em", "pmf_add_xreg_l2", "pmf_add_yreg_l2", "pmf_add_xreg_group", "pmf_add_yreg_group",
         "pmf_fit", "pmf_fit_lbfgs", "pmf_impute", "pmf_fsard_update_A"]


# ---- the shim --------------------------------------------------------------------------------------------------------
def strip_comments(src):
    """Drops `# ...` to the end of the line outside double-quoted strings; docstrings stay (they hold no code here)."""
    out = []
    for line in src.splitlines():
        in_str, esc, cut = False, False, len(line)
        for i, ch in enumerate(line):
            if esc:
                esc = False
            elif ch == "\\" and in_str:
                esc = True
            elif ch == '"':
                in_str = not in_str
            elif ch == "#" and not in_str:
                cut = i
                break
        out.append(line[:cut])
    return "\n".join(out)


def split_top(s):
    """Splits at top-level commas: brackets of every kind and double-quoted strings nest."""
    parts, depth, cur, in_str, esc = [], 0, [], False, False
    for ch in s:
        if in_str:
            cur.append(ch)
            if esc:
                esc = False
            elif ch == "\\":
                esc = True
            elif ch == '"':
                in_str = False
            continue
        if ch == '"':
            in_str = True
        elif ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    tail = "".join(cur).strip()
    if tail:
        parts.append(tail)
    return parts


def inner(s):
    s = s.strip()
    assert s.startswith("(") and s.endswith(")"), s
    return s[1:-1]


def ccalls(src):
    """[(line, [target, return type, type tuple, arg, ...])] for every `ccall(` of the source."""
    src = strip_comments(src)
    found = []
    for m in re.finditer(r"\bccall\(", src):
        depth, i, in_str = 1, m.end(), False
        while depth:
            ch = src[i]
            if ch == '"' and src[i - 1] != "\\":
                in_str = not in_str
            elif not in_str and ch == "(":
                depth += 1
            elif not in_str and ch == ")":
                depth -= 1
            i += 1
        found.append((src.count("\n", 0, m.start()) + 1, split_top(src[m.end():i - 1])))
    return found


def jl_class(t):
    t = t.strip()
    if re.fullmatch(r"(Ptr|Ref)\{.*\}", t):
        return "ptr"
    assert t in JL_CLASS, f"Julia type {t!r} has no C class here"
    return JL_CLASS[t]


def check_ccall(line, parts, protos):
    """Returns the bound name; raises AssertionError naming the line of the shim."""
    where = f"{SHIM.name}:{line}"
    assert len(parts) >= 3, (where, parts)
    target = split_top(inner(parts[0]))
    assert len(target) == 2, (where, parts[0])
    m = re.fullmatch(r":(pmf_\w+)", target[0])
    assert m, f"{where}: the function name {target[0]!r} is not a literal :pmf_* symbol (ccall cannot take a computed name)"
    name = m.group(1)
    assert name in protos, f"{where}: {name} is not declared in include/pmf_hip.h"
    ret, params = protos[name]
    assert parts[1] == ("Cstring" if name == "pmf_last_error" else "Cint"), (where, name, parts[1])
    assert jl_class(parts[1]) == ret, (where, name, parts[1])
    types = split_top(inner(parts[2]))
    args = parts[3:]
    assert len(types) == len(params), f"{where}: {name} takes {len(params)} parameters, the type tuple has {len(types)}"
    assert len(args) == len(params), f"{where}: {name} takes {len(params)} parameters, {len(args)} arguments are passed"
    for k, (t, c) in enumerate(zip(types, params)):
        assert jl_class(t) == c, f"{where}: {name} parameter {k + 1} is {c} in the header, {t} in the shim"
    return name


def jl_structs(src):
    src = strip_comments(src)
    out = {}
    for name, body in re.findall(r"^(?:mutable )?struct (\w+)\s*\n(.*?)^end", src, flags=re.S | re.M):
        out[name] = [(f, t) for f, t in re.findall(r"(\w+)::([\w{}]+)", body)]
    return out


@pytest.fixture(scope="module")
def shim():
    return SHIM.read_text()


def test_every_ccall_matches_its_prototype(shim):
    protos, _ = header()
    assert len(protos) >= 70 and protos["pmf_last_error"] == ("ptr", [])
    assert protos["pmf_stage_theta_delta_em"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr"])
    assert protos["pmf_set_data"] == ("i32", ["ptr", "ptr", "i64", "i64", "i32"])
    calls = ccalls(shim)
    assert len(calls) >= 40
    bound = {check_ccall(line, parts, protos) for line, parts in calls}
    missing = [n for n in BOUND if n not in bound]
    assert not missing, f"not bound in the shim: {missing}"


def test_the_scan_rejects_what_it_is_there_to_find():
    """The checker on small wrong snippets: a computed name, a short type tuple, a wrong class, a wrong return type."""
    protos, _ = header()
    bad = ['w = 1; chk(ccall((sym("l2"), LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Cfloat), ctx, w, p))',
           "ccall((:pmf_set_lr, LIB[]), Cint, (Ptr{Cvoid},), ctx, lr)",
           "ccall((:pmf_set_lr, LIB[]), Cint, (Ptr{Cvoid}, Cdouble), ctx, lr)",
           "ccall((:pmf_set_lr, LIB[]), Cvoid, (Ptr{Cvoid}, Cfloat), ctx, lr)",
           "ccall((:pmf_not_there, LIB[]), Cint, (Ptr{Cvoid},), ctx)"]
    for snippet in bad:
        (line, parts), = ccalls(snippet)
        with pytest.raises(AssertionError):
            check_ccall(line, parts, protos)
    good = 'x = f(a, "(") # ccall(\nccall((:pmf_set_lr, LIB[]), Cint, (Ptr{Cvoid}, Cfloat), context!(model; device=0), g(a, b)[1])'
    (line, parts), = ccalls(good)
    assert line == 2 and check_ccall(line, parts, protos) == "pmf_set_lr"


def test_structs_mirror_the_header(shim):
    _, cstructs = header()
    jstructs = jl_structs(shim)
    for jname, cname in STRUCTS.items():
        assert jname in jstructs, f"struct {jname} ({cname}) is missing from the shim"
        jf, cf = jstructs[jname], cstructs[cname]
        assert [f for f, _ in jf] == [f for f, _ in cf], (jname, jf, cf)
        for (f, jt), (_, cc) in zip(jf, cf):
            assert jl_class(jt) == cc, f"{jname}.{f}: {jt} in the shim, {cc} in {cname}"


def test_install_repoints_every_replaced_function(shim):
    body = strip_comments(shim)
    body = body[body.index("function install!"):]
    body = body[:body.index("\nend")]
    for name in INSTALLED:
        assert re.search(r"@eval PathMatFac " + re.escape(name) + r"\(", body), f"install! does not @eval {name}"
        assert re.search(r"^function " + re.escape(name) + r"\(", shim, flags=re.M), f"the shim does not define {name}"
    adam = shim[shim.index("function mf_fit!"):shim.index("function fit_lbfgs!")]
    assert "Flux.Optimise.Adam" in adam and "is_adam ? 1 : 0" in adam      # Adam reaches pmf_set_optimizer as kind 1
    assert "not been executed" in shim                                    # the note that no Julia ran stays
