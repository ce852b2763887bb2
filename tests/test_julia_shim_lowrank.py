"""Static check of the Julia shim's low-rank update methods against the C-ABI (no Julia in the image),
in the style of test_julia_shim_diag.py: the shim `ccall`s smlu_lowrank_set, smlu_lowrank_clear and
smlu_solve_lowrank with the header's argument counts, mirrors the header's record field for field, and
defines lowrank!, lowrank_clear! and ldiv_lowrank! (also on transpose(F) and F') on top of them."""
import re

from test_julia_shim import HEADER, SHIM, header_prototypes, shim_ccalls

LOWRANK = {"smlu_lowrank_set": 7, "smlu_lowrank_clear": 1, "smlu_solve_lowrank": 6}
JL_TYPE = {"int32_t": "Int32", "double": "Float64"}


def test_header_declares_the_entry_points():
    protos = header_prototypes()
    for name, nargs in LOWRANK.items():
        assert protos.get(name) == nargs, name
    assert protos.get("smlu_lowrank_set_device") == 7 and protos.get("smlu_solve_lowrank_device") == 6


def test_shim_ccalls_them_with_the_headers_argument_counts():
    protos = header_prototypes()
    seen = {}
    for syms, nargs in shim_ccalls(open(SHIM).read()):
        for s in syms:
            if s in LOWRANK:
                assert nargs == protos[s], f"{s}: shim passes {nargs} argument types, header has {protos[s]}"
                seen[s] = nargs
    assert sorted(seen) == sorted(LOWRANK)


def test_record_matches_the_header_field_for_field():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct smlu_lowrank_info \{(.*?)\} smlu_lowrank_info;", hdr, flags=re.S).group(1)
    want = []
    for t, names in re.findall(r"(\w+)\s+([\w,\s]+?);", body):
        want += [(nm.strip(), JL_TYPE[t]) for nm in names.split(",")]
    src = open(SHIM).read()
    jl = re.search(r"mutable struct LowrankInfo\n(.*?)\nend", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)::(\w+)", jl) == want


def test_methods_defined_and_exported():
    src = open(SHIM).read()
    assert re.search(r"^export .*\blowrank!, lowrank_clear!, ldiv_lowrank!", src, flags=re.M)
    assert re.search(r"\bfunction lowrank!\(F::ParallelSparseLU\{Float64\}, U::AbstractVecOrMat, V::AbstractVecOrMat\)", src)
    assert re.search(r"\blowrank_clear!\(F::ParallelSparseLU\)", src)
    # the three directions pass the header's SMLU_OP_N / SMLU_OP_T / SMLU_OP_H
    hdr = open(HEADER).read()
    ops = {nm: int(re.search(rf"#define\s+SMLU_OP_{nm}\s+(\d+)", hdr).group(1)) for nm in "NTH"}
    for who, arg, op in (("F::ParallelSparseLU", "F", ops["N"]), ("W::TransposedLU", "W.parent", ops["T"]),
                         ("W::AdjointLU", "W.parent", ops["H"])):
        pat = (rf"ldiv_lowrank!\(x::AbstractVector, {re.escape(who)}, b::AbstractVector; steps::Integer=-1\) =\s*"
               rf"_ldiv_lowrank!\(Int32\({op}\), x, {re.escape(arg)}, b, steps\)")
        assert re.search(pat, src), who
    # a singular capacitance matrix (status 1) throws, negative codes go through check
    assert "rc == 1 && throw(SingularException(0))" in src
    lim = int(re.search(r"#define\s+SMLU_LOWRANK_MAX\s+(\d+)", hdr).group(1))
    assert f"size(U, 2) <= {lim} ||" in src
