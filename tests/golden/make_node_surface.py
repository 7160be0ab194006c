"""Generates tests/golden/node_surface.json: the acados surface the reference's two ROS nodes
(crazyflie_controller/src/acados_mpc.cpp, acados_estimator.cpp) use, as data, so that
tests/test_node_surface.py checks this repository's drop-in headers and library without the nodes'
sources.  Run where the reference is checked out:

    python tests/golden/make_node_surface.py <reference checkout>

Per node and compile-time variant (the switches of acados_mpc.cpp:109-113, flipped in the
preprocessor input stream; the sources are read in place, never copied):
  includes  the acados / model headers the node includes, in order
  macros    identifiers the node uses that the drop-in headers define as macros
  globals   [type, name] of the acados globals the node defines (acados_mpc.cpp:76-84)
  calls     [function, [[argument type, value category], ...]] of every call into a function the
            drop-in headers declare (types as clang spells them before implicit conversions)
  members   [base type, "." or "->", field] of every field access on a drop-in struct
  undefined the acados-like symbols the node's object leaves undefined (g++ -c, nm -u)
  defined   the acados globals the node's object defines
The generator checks that the recorded surface compiles against the current headers.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INC = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat")]
CLANG = os.environ.get("CLANGXX", "/opt/rocm/llvm/bin/clang++")
OUT = os.path.join(HERE, "node_surface.json")

SWITCHES = ["SET_WEIGHTS", "WEIGHT_MATRICES", "FIXED_U0", "PUB_OPENLOOP_TRAJ"]
VARIANTS = {"acados_mpc.cpp": [{}, {"SET_WEIGHTS": 1, "WEIGHT_MATRICES": 1}, {"FIXED_U0": 1}, {"PUB_OPENLOOP_TRAJ": 1},
                               {k: 1 for k in SWITCHES}],
            "acados_estimator.cpp": [{}]}
ACADOS_LIKE = ("acados", "ocp_nlp", "sim_", "crazyflie", "nlp_", "forw_vde")
ACADOS_INCLUDE = re.compile(r'^\s*#\s*include\s*[<"]((?:acados|acados_c|blasfeo|crazyflie_model)/[^>"]+|acados_[a-z_]*crazyflie\.h)[>"]', re.M)


def variant_id(flips):
    return "+".join(flips) or "as-shipped"


def source(src_dir, name, flips):
    text = open(os.path.join(src_dir, name)).read()
    for k, v in flips.items():
        old = f"#define {k} {1 - v}"
        assert old in text, old
        text = text.replace(old, f"#define {k} {v}")
    return text


def ast(text):
    r = subprocess.run([CLANG, "-std=c++11", "-fsyntax-only", "-x", "c++", "-", *INC, "-Xclang", "-ast-dump=json"],
                       input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


def header_surface(includes):
    """Names of the functions and records the drop-in headers declare, and the macros they define."""
    tu = "".join(f'#include "{h}"\n' for h in includes)
    funcs, records = set(), set()

    def walk(n):
        k = n.get("kind")
        if k == "FunctionDecl" and not n.get("isImplicit"):
            funcs.add(n.get("name"))
        elif k in ("RecordDecl", "CXXRecordDecl", "TypedefDecl") and n.get("name"):
            records.add(n["name"])
        for c in n.get("inner", ()):
            walk(c)
    walk(ast(tu))
    base = subprocess.run(["g++", "-std=c++11", "-E", "-dM", "-x", "c++", "-"], input="", capture_output=True, text=True).stdout
    mine = subprocess.run(["g++", "-std=c++11", "-E", "-dM", "-x", "c++", "-", *INC], input=tu, capture_output=True, text=True,
                          check=True).stdout
    name = lambda ln: ln.split()[1].split("(")[0]
    macros = {name(ln) for ln in mine.splitlines()} - {name(ln) for ln in base.splitlines()}
    return funcs, records, macros


IMPLICIT = ("ImplicitCastExpr", "ExprWithCleanups", "MaterializeTemporaryExpr", "CXXBindTemporaryExpr", "ParenExpr")


def strip(e):
    while e.get("kind") in IMPLICIT and e.get("inner"):
        e = e["inner"][0]
    return e


def base_record(qual):
    return re.sub(r"\b(const|volatile|struct)\b|\*|&", " ", qual).split()[0] if qual.strip() else ""


def node_surface(text, funcs, records, macros):
    calls, members, globals_ = [], [], []
    tree = ast(text)

    def walk(n, top):
        k = n.get("kind")
        if k == "VarDecl" and top and base_record(n["type"]["qualType"]) in records and n.get("storageClass") != "extern":
            globals_.append([n["type"]["qualType"], n["name"]])
        if k == "CallExpr" and n.get("inner"):
            callee = strip(n["inner"][0])
            fn = callee.get("referencedDecl", {})
            if callee.get("kind") == "DeclRefExpr" and fn.get("kind") == "FunctionDecl" and fn.get("name") in funcs:
                args = [[strip(a)["type"]["qualType"], strip(a).get("valueCategory", "prvalue")] for a in n["inner"][1:]]
                calls.append([fn["name"], args])
        if k == "MemberExpr" and n.get("inner"):
            b = strip(n["inner"][0])
            bt = b["type"]["qualType"]
            if base_record(bt) in records:
                members.append([bt, "->" if n.get("isArrow") else ".", n["name"]])
        for c in n.get("inner", ()):
            walk(c, top and k == "TranslationUnitDecl")
    walk(tree, True)
    own = set(re.findall(r"^\s*#\s*define\s+(\w+)", text, re.M))
    used = set(re.findall(r"\b[A-Za-z_]\w*\b", re.sub(r"//[^\n]*|/\*.*?\*/", " ", text, flags=re.S)))
    uniq = lambda xs: [json.loads(s) for s in sorted({json.dumps(x) for x in xs})]
    return uniq(calls), uniq(members), uniq(globals_), sorted((used & macros) - own)


def object_symbols(text):
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "node.o")
        subprocess.run(["g++", "-std=c++11", "-c", "-w", "-x", "c++", "-", "-o", obj, *INC], input=text, text=True, check=True)
        undef = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-u", obj], text=True).splitlines()}
        defined = {ln.split()[-1] for ln in subprocess.check_output(["nm", "--defined-only", obj], text=True).splitlines()}
    like = lambda s: not s.startswith("_Z") and not s.startswith("__") and any(t in s for t in ACADOS_LIKE)
    return sorted(s for s in undef if like(s)), sorted(s for s in defined if like(s) or s in ("nlp_in", "nlp_out"))


def main(ref):
    src_dir = os.path.join(ref, "crazyflie_controller", "src")
    out = {}
    for name, variants in VARIANTS.items():
        out[name] = {}
        for flips in variants:
            text = source(src_dir, name, flips)
            includes = ACADOS_INCLUDE.findall(text)
            funcs, records, macros = header_surface(includes)
            calls, members, globals_, used_macros = node_surface(text, funcs, records, macros)
            undefined, defined = object_symbols(text)
            out[name][variant_id(flips)] = {"includes": includes, "macros": used_macros, "globals": globals_, "calls": calls,
                                            "members": members, "undefined": undefined, "defined": defined}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_node_surface import surface_tu          # the check the test runs: it must pass on the headers as they are
    for name, vs in out.items():
        for vid, s in vs.items():
            r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-x", "c++", "-", *INC[2:]], input=surface_tu(s),
                               capture_output=True, text=True)
            assert r.returncode == 0, (name, vid, r.stderr[-3000:])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, {n: {v: (len(s["calls"]), len(s["members"]), len(s["undefined"])) for v, s in vs.items()} for n, vs in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
