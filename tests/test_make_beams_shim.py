"""Static check of the Julia shim's torj_make_beams binding (torj.jl_amd/julia/TorJHIP.jl)
against include/torj_hip.h, as tests/test_julia_shim.py checks the other bindings: the call
passes three struct pointers (torj_launcher, torj_beam_result, torj_beams_rays), so it is
written with typed pointers through the @ccall macro, and this file checks it -- the
argument count and each argument's type against the prototype, and the three Julia structs'
fields against the C structs' in order and type."""
import re

from test_julia_shim import HEADER, JL2C, SHIM, _balanced, _norm_c, _split_top, header_prototypes

STRUCTS = {"Launcher": "torj_launcher", "BeamResult": "torj_beam_result", "BeamsRays": "torj_beams_rays"}
TYPES = dict(JL2C)
TYPES.update({"Ptr{Launcher}": {"torj_launcher*"}, "Ptr{BeamResult}": {"torj_beam_result*"},
              "Ptr{BeamsRays}": {"torj_beams_rays*"}})


def shim_source():
    return re.sub(r"#[^\n]*", "", open(SHIM).read())


def c_fields(name):
    """[(field, normalised C type)] of `typedef struct { ... } name;`, a star counted with its own declarator"""
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", h)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base, names = re.match(r"((?:const\s+)?\w+)\s*(.*)", decl).groups()
        for nm in names.split(","):
            out.append((nm.replace("*", "").strip(), _norm_c(base + "*" * nm.count("*"))))
    return out


def jl_fields(name):
    m = re.search(r"struct " + name + r"\s*\n(.*?)\nend", shim_source(), flags=re.S)
    assert m, name
    return re.findall(r"(\w+)::([\w{}]+)", m.group(1))


def macro_call():
    """the @ccall of torj_make_beams -> (return type, [(argument, type)])"""
    src = shim_source()
    m = re.search(r"@ccall\s+libtorj\.torj_make_beams\(", src)
    assert m, "no @ccall of torj_make_beams in the shim"
    i = m.end() - 1
    j = _balanced(src, i)
    ret = re.match(r"::(\w+)", src[j:]).group(1)
    args = []
    for a in _split_top(src[i + 1:j - 1]):
        k = a.rindex("::")
        args.append((a[:k].strip(), a[k + 2:].strip()))
    return ret, args


def test_structs_match_header():
    for jl, c in STRUCTS.items():
        jf, cf = jl_fields(jl), c_fields(c)
        assert [n for n, _ in jf] == [n for n, _ in cf], jl
        for (n, jt), (_, ct) in zip(jf, cf):
            assert jt in JL2C, f"{jl}.{n}: unmapped Julia type {jt}"
            assert ct in JL2C[jt], f"{jl}.{n}: Julia {jt} vs C {ct}"


def test_call_matches_header():
    ret, args = macro_call()
    c_ret, c_params = header_prototypes()["torj_make_beams"]
    assert c_ret in TYPES[ret]
    assert len(args) == len(c_params) == 14
    for k, ((_, jt), ct) in enumerate(zip(args, c_params)):
        assert jt in TYPES, f"arg {k}: unmapped Julia type {jt}"
        assert ct in TYPES[jt], f"arg {k}: Julia {jt} vs C {ct}"


def test_checker_catches_a_swapped_field():
    """the check itself: the C struct's field order is what is compared"""
    cf = c_fields("torj_launcher")
    assert [t for _, t in cf] == ["double"] * 8 + ["int"] * 2
    assert cf[3][0] == "steering_angle_tor" and cf[4][0] == "steering_angle_pol"
    assert c_fields("torj_beams_rays")[6] == ("entry_status", "int*")
    assert c_fields("torj_beams_rays")[8:10] == [("status", "int*"), ("steps", "int*")]


def test_arguments_that_may_be_null_are_ptr():
    """The shim passes C_NULL for plasmas, dP_dV, res and rays (one plasma; the count-only call).
    A Ptr{T} argument converts C_NULL to a null pointer; a Ref{T} one would try to build a T from
    it and throw."""
    _, args = macro_call()
    by_name = {a: t for a, t in args}
    for a in ("hs", "dP_dV", "res", "rays"):
        assert by_name[a].startswith("Ptr{"), f"{a}::{by_name[a]}"
