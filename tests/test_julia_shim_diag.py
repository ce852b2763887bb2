"""Static check of the Julia shim's determinant / condition-estimate methods against the C-ABI (no
Julia in the image), in the style of test_julia_shim.py: the shim `ccall`s smlu_logabsdet,
smlu_logabsdet_z and smlu_rcond with the header's argument counts, and defines the LinearAlgebra
methods on top of them."""
import re

from test_julia_shim import HEADER, SHIM, header_prototypes, shim_ccalls

DIAG = {"smlu_logabsdet": 3, "smlu_logabsdet_z": 3, "smlu_rcond": 5}


def test_header_declares_the_three_entry_points():
    protos = header_prototypes()
    for name, nargs in DIAG.items():
        assert protos.get(name) == nargs, name


def test_shim_ccalls_them_with_the_headers_argument_counts():
    protos = header_prototypes()
    seen = {}
    for syms, nargs in shim_ccalls(open(SHIM).read()):
        for s in syms:
            if s in DIAG:
                assert nargs == protos[s], f"{s}: shim passes {nargs} argument types, header has {protos[s]}"
                seen[s] = nargs
    assert sorted(seen) == sorted(DIAG)


def test_linear_algebra_methods_defined():
    src = open(SHIM).read()
    for fn in ("logabsdet", "logdet", "det", "cond"):
        assert re.search(rf"\bLinearAlgebra\.{fn}\(F::ParallelSparseLU", src), fn
    # the norm argument is the header's SMLU_NORM_ONE / SMLU_NORM_INF
    hdr = open(HEADER).read()
    one = int(re.search(r"#define\s+SMLU_NORM_ONE\s+(\d+)", hdr).group(1))
    inf = int(re.search(r"#define\s+SMLU_NORM_INF\s+(\d+)", hdr).group(1))
    assert f"Int32(p == 1 ? {one} : {inf})" in src
    # cond(F) without p would silently differ from LinearAlgebra's 2-norm default: no default here
    assert re.search(r"LinearAlgebra\.cond\(F::ParallelSparseLU, p::Real\)", src)
