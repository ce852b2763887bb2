"""Static check of the Julia shim's batched refined solve against the C-ABI (no Julia in the image),
in the style of test_julia_shim_diag.py: ldiv_refined! `ccall`s smlu_solve_refined_multi with the
header's argument count, its RefineInfo record has the header's fields in order, and the method is
defined and exported for F, transpose(F) and F'."""
import re

from test_julia_shim import C2JL, HEADER, SHIM, _header, header_prototypes, shim_ccalls

NAME = "smlu_solve_refined_multi"


def test_header_declares_the_entry_points():
    protos = header_prototypes()
    assert protos.get(NAME) == 9
    assert protos.get(NAME + "_device") == 9


def test_shim_ccalls_it_with_the_headers_argument_count():
    protos = header_prototypes()
    seen = [nargs for syms, nargs in shim_ccalls(open(SHIM).read()) if NAME in syms]
    assert seen == [protos[NAME]]


def test_record_matches_the_header():
    body = re.search(r"typedef struct smlu_refine_info \{(.*?)\} smlu_refine_info;", _header(), flags=re.S).group(1)
    hdr = [(name, C2JL[ctype]) for ctype, name in re.findall(r"(\w+)\s+(\w+)\s*;", body)]
    assert [n for n, _ in hdr] == ["steps", "stop", "berr", "resid"]
    src = open(SHIM).read()
    jl = re.search(r"^struct RefineInfo;(.*?)end$", src, flags=re.M).group(1)
    assert re.findall(r"(\w+)::(\w+)", jl) == hdr
    # the record is handed over as one per column, and the op / step arguments as Int32
    assert "Vector{RefineInfo}(undef, size(B, 2))" in src
    assert "(Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Tf}, Int64, Ptr{Tf}, Int64, Ptr{RefineInfo})" in src


def test_methods_defined_and_exported():
    src = open(SHIM).read()
    assert re.search(r"^export .*\bldiv_refined!", src, flags=re.M)
    hdr = open(HEADER).read()
    ops = {k: int(re.search(rf"#define\s+SMLU_OP_{k}\s+(\d+)", hdr).group(1)) for k in "NTH"}
    for arg, op, parent in (("F::ParallelSparseLU", ops["N"], "F"), ("W::TransposedLU", ops["T"], "W.parent"),
                            ("W::AdjointLU", ops["H"], "W.parent")):
        pat = (rf"ldiv_refined!\(X::AbstractMatrix, {re.escape(arg)}, B::AbstractMatrix; steps::Integer=-1\) =\s*"
               rf"_ldiv_refined!\(Int32\({op}\), X, {re.escape(parent)}, B, steps\)")
        assert re.search(pat, src), arg
    assert "return [i.steps for i in info], [i.berr for i in info]" in src
