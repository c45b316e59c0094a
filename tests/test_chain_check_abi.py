"""CPU: one table of rejected arguments for the six whole-graph propagation calls and
appnp_plan_create_solve (include/ppnp_amd.h), which share one argument check
(ppnp_amd/csrc/appnp_propagate.hip check_chain).

Every row is one bad argument and the code each entry point returns for it.  The codes were
recorded from the library as it was when each family still had a check of its own, so the table
pins that the entry points agree with that library, and with each other, on what is rejected and
in which order.  No call reaches a device: unless a row names its own graph it runs on an empty
one (n = 0) with null operands, where a call whose arguments are all valid returns APPNP_OK
("valid, nothing to do") before it looks at a pointer -- so a code other than OK comes from the
row's argument, and from a check that precedes the empty shape.  The last rows, on a graph with
rows, end at the pointer checks.  The graph is the host-only stand-in of tests/test_poly_abi.py.
Cases that need a device-side graph (a transpose that is held, in == out, ld < f, the
workspace) are in the GPU suites and in tests/test_capi_trace.py.
"""

import ctypes as C

import pytest

from ppnp_amd import _lib as L

OK, E, NS = L.APPNP_OK, L.APPNP_EINVAL, L.APPNP_ENOTSUP
NA = None  # not called: nothing in the row stops this entry point short of the device

ENTRY_POINTS = ("appnp_propagate", "appnp_propagate_bwd", "appnp_solve", "appnp_solve_bwd",
                "appnp_poly", "appnp_poly_bwd", "appnp_plan_create_solve")


class _GraphHead(C.Structure):
    """The leading fields of struct appnp_graph (ppnp_amd/csrc/appnp_internal.h), followed by
    zero bytes for the rest (every pointer NULL, no transpose)."""
    _fields_ = [("n", C.c_int64), ("row_lo", C.c_int64), ("row_hi", C.c_int64),
                ("nnz_hat", C.c_int64), ("nnz_local", C.c_int64), ("nnz_remote", C.c_int64),
                ("mode", C.c_int), ("symmetric", C.c_int), ("rest", C.c_char * 2048)]


def _graph(n=0, row_lo=0, row_hi=None, mode=0, symmetric=1):
    return _GraphHead(n=n, row_lo=row_lo, row_hi=n if row_hi is None else row_hi, mode=mode,
                      symmetric=symmetric)


P, Q, COEF = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)  # never dereferenced


def _call(name, g=_graph(), f=7, dtype=L.F32, steps=4, alpha=0.1, p_drop=0.0, coef=COEF,
          operands=False):
    """``name`` with the row's arguments; one the entry point does not take is dropped.  The
    workspace is null, and so are the operands unless the row gives them."""
    lib = L.load()
    gp = None if g is None else C.cast(C.pointer(g), C.c_void_p)
    X, Y = (P, Q) if operands else (None, None)
    head = (gp, X, 8, Y, 8, f, dtype, steps)
    if name in ("appnp_propagate", "appnp_propagate_bwd"):
        return getattr(lib, name)(*head, alpha, p_drop, 0, None, 0, None)
    if name in ("appnp_solve", "appnp_solve_bwd"):
        return getattr(lib, name)(*head, alpha, None, 0, None)
    if name == "appnp_poly":
        return lib.appnp_poly(*head, coef, None, 0, None)
    if name == "appnp_poly_bwd":
        return lib.appnp_poly_bwd(gp, X, 8, None, 8, Y, 8, None, f, dtype, steps, coef, None, 0,
                                  None)
    out = C.c_void_p(0xbad0)
    rc = lib.appnp_plan_create_solve(*head, alpha, None, 0, C.byref(out))
    assert out.value is None  # a rejected plan leaves no handle
    return rc


# appnp_plan_create_solve is called only where appnp_solve rejects the row: arguments it accepts
# take it on to the capture stream, which needs a device.  So would the last row take every call
# but appnp_poly's.
#
#   case                           arguments                       prop prop_bwd solve solve_bwd
#                                                                  poly poly_bwd plan_solve
CASES = [
    ("nothing wrong",              {},                             (OK, OK, OK, OK, OK, OK, NA)),
    ("null graph",                 {"g": None},                    (E, E, E, E, E, E, E)),
    ("f < 0",                      {"f": -1},                      (E, E, E, E, E, E, E)),
    ("f > INT32_MAX",              {"f": 2**31},                   (E, E, E, E, E, E, E)),
    ("steps = -1",                 {"steps": -1},                  (E, E, E, E, E, E, E)),
    ("steps = 0",                  {"steps": 0},                   (OK, OK, E, E, OK, OK, E)),
    ("steps = APPNP_POLY_MAX_K",   {"steps": 1024},                (OK, OK, OK, OK, OK, OK, NA)),
    ("steps > APPNP_POLY_MAX_K",   {"steps": 1025},                (OK, OK, OK, OK, E, E, NA)),
    ("steps = 2^20",               {"steps": 2**20},               (OK, OK, OK, OK, E, E, NA)),
    ("steps > 2^20",               {"steps": 2**20 + 1},           (OK, OK, E, E, E, E, E)),
    ("dtype = 2",                  {"dtype": 2},                   (E, E, E, E, E, E, E)),
    ("dtype = -1",                 {"dtype": -1},                  (E, E, E, E, E, E, E)),
    ("alpha < 0",                  {"alpha": -0.1},                (E, E, E, E, OK, OK, E)),
    ("alpha > 1",                  {"alpha": 1.5},                 (E, E, E, E, OK, OK, E)),
    ("alpha NaN",                  {"alpha": float("nan")},        (E, E, E, E, OK, OK, E)),
    ("alpha = 0",                  {"alpha": 0.0},                 (OK, OK, E, E, OK, OK, E)),
    ("alpha = 1",                  {"alpha": 1.0},                 (OK, OK, OK, OK, OK, OK, NA)),
    ("p_drop = 1",                 {"p_drop": 1.0},                (E, E, OK, OK, OK, OK, NA)),
    ("p_drop < 0",                 {"p_drop": -0.1},               (E, E, OK, OK, OK, OK, NA)),
    ("bf16",                       {"dtype": L.BF16},              (OK, OK, NS, NS, NS, NS, NS)),
    # EINVAL before ENOTSUP: what is wrong is reported before what is not offered
    ("bf16 and steps = -1",        {"dtype": L.BF16, "steps": -1}, (E, E, E, E, E, E, E)),
    ("bf16 and alpha = 0",         {"dtype": L.BF16, "alpha": 0.0},
     (OK, OK, E, E, NS, NS, E)),
    ("bf16 and held rows only",    {"dtype": L.BF16, "g": _graph(n=100, row_hi=50)},
     (E, E, E, E, E, E, E)),
    ("held rows only",             {"g": _graph(n=100, row_lo=10)}, (E, E, E, E, E, E, E)),
    # A_hat^T: A_hat itself for 'sym' on an undirected graph, else the transpose, which the
    # stand-in does not hold; the solver takes undirected graphs only
    ("rw, no transpose",           {"g": _graph(mode=1)},          (OK, NS, OK, NS, OK, NS, NA)),
    ("directed, no transpose",     {"g": _graph(symmetric=0)},     (OK, NS, NS, NS, OK, NS, NS)),
    ("directed rw, no transpose",  {"g": _graph(mode=1, symmetric=0)},
     (OK, NS, NS, NS, OK, NS, NS)),
    ("held rows of an rw graph",   {"g": _graph(n=100, row_hi=50, mode=1)},
     (E, E, E, E, E, E, E)),
    # the pointers come last: on an empty shape even a null coef is not looked at ...
    ("null coef, empty graph",     {"coef": None},                 (OK, OK, OK, OK, OK, OK, NA)),
    ("f = 0 on a graph with rows", {"g": _graph(n=100), "f": 0, "coef": None},
     (OK, OK, OK, OK, OK, OK, NA)),
    # ... and on a graph with rows the null operands are EINVAL for every call (so a null coef
    # is, too; appnp_plan_create_solve checks them before it creates its stream)
    ("null operands and coef",     {"g": _graph(n=100), "coef": None}, (E, E, E, E, E, E, E)),
    ("null operands, bf16",        {"g": _graph(n=100), "dtype": L.BF16},
     (E, E, NS, NS, NS, NS, NS)),
    ("null coef beside operands",  {"g": _graph(n=100), "coef": None, "operands": True},
     (NA, NA, NA, NA, E, E, NA)),
]


assert all(len(want) == len(ENTRY_POINTS) for _, _, want in CASES)


@pytest.mark.parametrize("entry,args,want", [
    pytest.param(entry, args, want[i], id=f"{entry}-{name}")
    for name, args, want in CASES for i, entry in enumerate(ENTRY_POINTS) if want[i] is not NA])
def test_rejected_arguments_table(entry, args, want):
    assert _call(entry, **args) == want
