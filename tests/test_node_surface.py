"""Row N4: the reference's two ROS nodes against this repository's drop-in
headers and library.  What the nodes use of acados -- the headers they include, the macros, the
globals they define, every call with its argument types, every struct field, the symbols their
objects leave undefined -- is stored in tests/golden/node_surface.json (extracted from the
reference's sources by tests/golden/make_node_surface.py; the sources themselves are never copied).
The drop-in headers must declare all of it with compatible types, and libacados_solver_crazyflie.so
must export every such symbol.

With CFNMPC_REFERENCE_DIR set to a checkout of the reference, the nodes' own sources are in addition
parsed and compiled in place against the drop-in headers (ROS / Eigen / boost / generated message
headers: declaration-only stand-ins under tests/stubs/, see its README).  Compile-only: nothing is
linked into a program or executed, and nothing here is an oracle."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.path.join(os.environ["CFNMPC_REFERENCE_DIR"], "crazyflie_controller", "src") if os.environ.get("CFNMPC_REFERENCE_DIR") else None
INC = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat")]
SHIM = os.path.join(ROOT, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so")
SURFACE = os.path.join(ROOT, "tests", "golden", "node_surface.json")

# compile-time switches of acados_mpc.cpp:109-113, all 0/1 in the reference; flipped in the
# preprocessor input stream (the file itself is never copied or modified)
VARIANTS = [{}, {"SET_WEIGHTS": 1, "WEIGHT_MATRICES": 1}, {"FIXED_U0": 1}, {"PUB_OPENLOOP_TRAJ": 1}]


def _variant_id(flips):
    return "+".join(flips) or "as-shipped"


def _surface(name, flips):
    with open(SURFACE) as f:
        return json.load(f)[name][_variant_id(flips)]


def _source(name, flips):
    """The node's own source with the switches flipped, or None without CFNMPC_REFERENCE_DIR."""
    if REF_SRC is None:
        return None
    text = open(os.path.join(REF_SRC, name)).read()
    for k, v in flips.items():
        old = f"#define {k} {1 - v}"
        assert old in text, old
        text = text.replace(old, f"#define {k} {v}")
    return text


def surface_tu(s):
    """A translation unit that uses the drop-in headers exactly as the node does (node_surface.json): same includes, every
    macro it uses defined, its globals defined with their types, every call type-checked with the node's argument types and
    value categories, every field access resolved (decltype: unevaluated, nothing runs)."""
    ref = {"lvalue": "&", "xvalue": "&&", "prvalue": ""}
    lines = [f'#include "{h}"' for h in s["includes"]] + ["#include <utility>"]
    for m in s["macros"]:
        lines += [f"#ifndef {m}", f'#error "{m}: not defined by the drop-in headers"', "#endif"]
    lines += [f"{t} {n};" for t, n in s["globals"]]
    lines.append("namespace node_surface {")
    for i, (fn, args) in enumerate(s["calls"]):
        lines += [f"using A{i}_{j} = {t};" for j, (t, _c) in enumerate(args)]
        vals = ", ".join(f"std::declval<A{i}_{j}{ref[c]}>()" for j, (_t, c) in enumerate(args))
        lines.append(f"using R{i} = decltype({fn}({vals}));")
    for i, (bt, op, field) in enumerate(s["members"]):
        lines += [f"using B{i} = {bt};", f"using M{i} = decltype(std::declval<B{i}&>(){op}{field});"]
    lines.append("}")
    return "\n".join(lines) + "\n"


def _parses(name, flips):
    s = _surface(name, flips)
    assert s["includes"] and s["calls"], s          # the fixture is not empty
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-x", "c++", "-", *INC[2:]], input=surface_tu(s),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = _source(name, flips)
    if text is not None:
        r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-x", "c++", "-", *INC], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("flips", VARIANTS, ids=lambda f: "+".join(f) or "as-shipped")
def test_nmpc_node_parses_against_dropin_headers(flips):
    """crazyflie_controller/src/acados_mpc.cpp (includes :61-73, globals :76-84, calls :225, :418,
    :581-625 and, with the switches on, "W" :596-602, "lbu"/"ubu" :605-608, the open-loop getters :679-682)."""
    _parses("acados_mpc.cpp", flips)


def test_estimator_node_parses_against_dropin_headers():
    """crazyflie_controller/src/acados_estimator.cpp (includes :66-76, sim calls :237, :573-593)."""
    _parses("acados_estimator.cpp", {})


@pytest.mark.parametrize("name,flips", [("acados_mpc.cpp", {}), ("acados_mpc.cpp", {"SET_WEIGHTS": 1, "WEIGHT_MATRICES": 1, "FIXED_U0": 1, "PUB_OPENLOOP_TRAJ": 1}),
                                        ("acados_estimator.cpp", {})])
def test_node_objects_resolve_against_the_dropin_library(tmp_path, name, flips):
    """Object file only (never linked into a program, never run): every symbol the node's object
    leaves undefined that is not libc / libstdc++ must be exported by the drop-in library, and the
    acados globals the node DEFINES (acados_mpc.cpp:76-84) must be the ones the library expects."""
    if not os.path.exists(SHIM):
        pytest.skip("drop-in library not built (python -c 'import __graft_entry__ as g; g.build()')")
    s = _surface(name, flips)
    acados_like, defined = set(s["undefined"]), set(s["defined"])
    text = _source(name, flips)
    if text is not None:   # the node's own object, compiled here: the stored symbols must be what it leaves undefined / defines
        obj = tmp_path / "node.o"
        r = subprocess.run(["g++", "-std=c++11", "-c", "-w", "-x", "c++", "-", "-o", str(obj), *INC], input=text,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        undef = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-u", str(obj)], text=True).splitlines()}
        live = {s for s in undef if not s.startswith("_Z") and not s.startswith("__") and
                any(t in s for t in ("acados", "ocp_nlp", "sim_", "crazyflie", "nlp_", "forw_vde"))}
        assert live == acados_like, sorted(live ^ acados_like)
        defined = {ln.split()[-1] for ln in subprocess.check_output(["nm", "--defined-only", str(obj)], text=True).splitlines()}
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", SHIM], text=True).splitlines()}
    assert acados_like, s
    missing = sorted(acados_like - exported)
    assert not missing, missing
    must = {"acados_mpc.cpp": {"acados_create", "acados_solve", "ocp_nlp_constraints_model_set", "ocp_nlp_cost_model_set",
                               "ocp_nlp_out_get"},
            "acados_estimator.cpp": {"crazyflie_acados_sim_create", "crazyflie_acados_sim_solve", "sim_in_set", "sim_out_get"}}[name]
    assert must <= acados_like, sorted(must - acados_like)
    if name == "acados_mpc.cpp":
        assert {"nlp_in", "nlp_out", "nlp_solver", "nlp_opts", "nlp_solver_plan", "nlp_config", "nlp_dims", "forw_vde_casadi"} <= defined
