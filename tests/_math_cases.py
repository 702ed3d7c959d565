"""bb_debug_math (barbay.jl_amd/csrc/bb_mathprobe.h): the functions of csrc/bb_math.h and the Box-Muller step of bb_block.h as the
kernels call them, at the stored arguments of tests/golden/math_<fn>.npz against their 50-digit values
(tests/golden/make_math_golden.py) -- the cases the emulation test (host build of the header: exact seeds, C Horner loops, glibc
ldexp / frexp) and the GPU test (hardware seeds, v_fma_f64 blocks on scalar coefficients, __constant__ tables, device ldexp /
frexp) share.

Bounds: the ones tests/test_bb_math.py asserts for the host build, unchanged.  "rel" is |got - exact| / max(|exact|, 2^-1022), so a
subnormal result is judged against the smallest normal; "abs" is |got - exact|.  Box-Muller: |got - exact| <= 1e-15 r with r the
exact radius sqrt(-2 ln u1): half of log's 6e-16 through the square root, sqrt's and sincospi's 3e-16 each and one rounding of
the product.  Every stored argument is asserted.  exp_nonpos and log_1to2 must also equal exp and log bit for bit at their
arguments, as the header says.

Measured, largest error over a function's stored arguments, host emulation / MI355X, next to the bound; and at how many arguments
the device's result differs bitwise from the emulation's (the seeds differ: 2^-24 on the device, correctly rounded on the host):

function      arguments   emulation      MI355X      bound          differing bitwise
exp                5993    1.567e-16   1.567e-16    4e-16 rel          0
exp_nonpos         3171    1.567e-16   1.567e-16    4e-16 rel          0   (= exp bit for bit on both)
log                5483    2.546e-16   2.546e-16    6e-16 rel          1
log_1to2           1402    2.538e-16   2.538e-16    6e-16 rel          0   (= log bit for bit on both)
rcp               10018    1.110e-16   1.110e-16    3e-16 rel          0
div                4962    1.110e-16   1.110e-16    3e-16 rel          0
sqrt               7230    1.110e-16   1.110e-16    3e-16 rel          0
softplus           3261    3.892e-16   3.892e-16    1e-15 rel          0
sigmoid            3261    2.989e-16   2.989e-16    1e-15 rel          0
sinpi              1508    1.498e-16   1.498e-16    3e-16 abs          0
cospi              1508    1.177e-16   1.177e-16    3e-16 abs          0
normal0            3368    2.489e-16   2.489e-16    1e-15 r            0
normal1            3368    2.517e-16   2.517e-16    1e-15 r            0
(sqrt before its branch for x < 2^-900 (bb_math.h), on the 6924 arguments of that time: emulation 1.387e-16, MI355X 4.441e-16 at
 x = 2.07e-317 with 33 subnormal arguments over the bound and 40 differing bitwise -- the residual x - g^2 of the final correction
 has no bits below 2^-1074, so the device kept the Goldschmidt iteration's own error, which the host's exact seed does not have.
 The 306 tiny and subnormal arguments at the end of the sqrt table were added with the fix.)
"""
import ctypes as C
import functools
import glob
import os

import numpy as np

from conftest import make_engine
from barbay_jl_amd import _capi
from oracle import fixtures

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TWO_IN = ("div", "box_muller")
# fn -> ((result name, kind of bound, bound), ...)
BOUNDS = {
    "exp": (("exp", "rel", 4e-16),),
    "exp_nonpos": (("exp_nonpos", "rel", 4e-16),),
    "log": (("log", "rel", 6e-16),),
    "log_1to2": (("log_1to2", "rel", 6e-16),),
    "rcp": (("rcp", "rel", 3e-16),),
    "div": (("div", "rel", 3e-16),),
    "sqrt": (("sqrt", "rel", 3e-16),),
    "softplus_sigmoid": (("softplus", "rel", 1e-15), ("sigmoid", "rel", 1e-15)),
    "sincospi": (("sinpi", "abs", 3e-16), ("cospi", "abs", 3e-16)),
    "box_muller": (("normal0", "radius", 1e-15), ("normal1", "radius", 1e-15)),
}
FNS = tuple(BOUNDS)
TWIN = {"exp_nonpos": "exp", "log_1to2": "log"}          # the same bits as ... at the same argument
MIN_NORMAL = 2.0 ** -1022


@functools.lru_cache(maxsize=None)
def load(fn):
    """The golden of `fn`, its parts joined in order; read-only arrays."""
    paths = [os.path.join(GOLD, f"math_{fn}.npz")]
    paths += sorted(glob.glob(os.path.join(GOLD, f"math_{fn}_p[0-9]*.npz")), key=lambda p: int(p[:-4].rsplit("_p", 1)[1]))
    parts = [np.load(p) for p in paths]
    d = {k: np.concatenate([p[k] for p in parts]) for k in parts[0].files}
    for v in d.values():
        v.setflags(write=False)
    return d


def handle(lib, **kw):
    return make_engine(fixtures.load("data001_single"), lib, **kw)


def evaluate(lib, fn, x, y=None, **kw):
    with handle(lib, **kw) as e:
        return e.debug_math(fn, x, y)


def golden_args(fn):
    g = load(fn)
    return g["x"], (g["y"] if fn in TWO_IN else None)


def errors(fn, out):
    """Per result of `fn`: the error of out[k] at every golden argument, in the units of its bound (rel / abs / radius)."""
    g = load(fn)
    res = []
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (_, kind, _) in enumerate(BOUNDS[fn]):
            hi, lo, scale = g[f"hi{k}"], g[f"lo{k}"], np.ldexp(1.0, g[f"shift{k}"].astype(np.int32))
            err = np.abs((out[k] - hi) * scale - lo)                    # (got - hi: exact for any got within a factor 2 of hi)
            if kind == "rel":
                err = err / (np.maximum(np.abs(hi), MIN_NORMAL) * scale)
            else:
                err = err / scale
            res.append(err)
    return res


def _same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)


def check(lib, fn, label, other=None):
    """Every golden argument of `fn` within its bound on `lib`; the figures are printed first.  `other`: a second library (the
    emulation next to the device) whose results are compared bit for bit -- reported, not asserted: the seeds differ."""
    g = load(fn)
    x, y = golden_args(fn)
    out = evaluate(lib, fn, x, y)
    errs = errors(fn, out)
    for k, (name, kind, bound) in enumerate(BOUNDS[fn]):
        e = errs[k]
        if kind == "radius":                                             # in units of r (r = 0: the result must be exact)
            with np.errstate(invalid="ignore", divide="ignore"):
                e = np.where(e == 0.0, 0.0, e / g["r"])
        e = np.where(np.isnan(e), np.inf, e)
        worst = int(np.argmax(e))
        print(f"{label:9s} {name:10s} n {x.size:5d}  max {kind} error {e[worst]:.3e} (bound {bound:g}) at x = {x[worst]!r}"
              + (f", y = {y[worst]!r}" if y is not None else "") + f"; over the bound: {int((e > bound).sum())}")
    if other is not None:
        o2 = evaluate(other, fn, x, y)
        for k, (name, _, _) in enumerate(BOUNDS[fn]):
            print(f"{label:9s} {name:10s} differs bitwise from the other build at {int((~_same_bits(out[k], o2[k])).sum())} of {x.size}")
    for k, (name, kind, bound) in enumerate(BOUNDS[fn]):
        lim = bound * g["r"] if kind == "radius" else bound
        assert np.all(errs[k] <= lim), (name, float(np.nanmax(errs[k])))
    if fn in TWIN:
        t0, _ = evaluate(lib, TWIN[fn], x)
        assert np.all(_same_bits(out[0], t0)), (fn, x[~_same_bits(out[0], t0)][:5])
    check_specials(lib, fn, out)


def check_specials(lib, fn, out):
    """The values that must be exact."""
    g = load(fn)
    x = g["x"]
    if fn in ("exp", "exp_nonpos"):
        a = np.array([-800.0, 800.0] if fn == "exp" else [-800.0, -1e4])
        got, _ = evaluate(lib, fn, a)
        assert got[0] == 0.0 and (got[1] == np.inf if fn == "exp" else got[1] == 0.0), got
    if fn == "log":
        assert (x == 1.0).any() and np.all(out[0][x == 1.0] == 0.0)
    if fn == "sqrt":
        assert (x == 0.0).any() and np.all(out[0][x == 0.0] == 0.0)
    if fn == "div":
        assert (x == 0.0).sum() == 2 and np.all(out[0][x == 0.0] == 0.0)
    if fn == "box_muller":
        one = (x >> np.uint64(11)) == np.uint64(2 ** 53 - 1)                 # u1 = 1
        assert one.sum() >= 24 and np.all(g["r"][one] == 0.0)
        assert np.all(out[0][one] == 0.0) and np.all(out[1][one] == 0.0)


def check_errors(lib):
    """BB_ERR_INVALID for an unknown function, a negative n and every missing pointer the function needs; n = 0 succeeds and
    writes nothing."""
    x, y, o0, o1 = (np.full(4, v) for v in (1.5, 3.0, -7.0, -7.0))
    p = lambda a: a.ctypes.data_as(_capi._dp)
    with handle(lib) as e:
        call = lambda *a: lib.bb_debug_math(e._h, *a)
        assert call(-1, 4, p(x), p(y), p(o0), p(o1)) == -1
        assert call(len(_capi.BB_MATH_FN), 4, p(x), p(y), p(o0), p(o1)) == -1
        assert lib.bb_debug_math(None, 0, 4, p(x), p(y), p(o0), p(o1)) == -1
        for name, code in _capi.BB_MATH_FN.items():
            two_in = name in TWO_IN
            two_out = len(BOUNDS[name]) == 2
            assert call(code, -1, p(x), p(y), p(o0), p(o1)) == -1, name
            assert call(code, 4, None, p(y), p(o0), p(o1)) == -1, name
            assert call(code, 4, p(x), p(y), None, p(o1)) == -1, name
            assert call(code, 4, p(x), None, p(o0), p(o1)) == (-1 if two_in else 0), name
            assert call(code, 4, p(x), p(y), p(o0), None) == (-1 if two_out else 0), name
            assert b"" != lib.bb_last_error()
            o0[:], o1[:] = -7.0, -7.0
            assert call(code, 0, p(x), p(y), p(o0), p(o1)) == 0, name
            assert np.all(o0 == -7.0) and np.all(o1 == -7.0)
        with np.testing.assert_raises(_capi.BarBayHipError):
            e.debug_math(99, x)
        a, b = e.debug_math("rcp", np.empty(0))
        assert a.shape == (0,) and b is None
        assert sorted(_capi.BB_MATH_FN) == sorted(FNS)


def check_group_handle(lib):
    """A device_ids = [0, 0] group handle (shard 0 answers) against a single handle, byte for byte."""
    for fn in ("exp", "div", "softplus_sigmoid", "box_muller"):
        x, y = golden_args(fn)
        x, y = x[:1500], (None if y is None else y[:1500])
        a = evaluate(lib, fn, x, y, device_ids=[0, 0])
        b = evaluate(lib, fn, x, y)
        for u, v in zip(a, b):
            assert (u is None and v is None) or u.tobytes() == v.tobytes(), fn


def check_buffer_reuse(lib):
    """BUF_DBG across calls on ONE handle: a large probe call, a small bb_debug_normals call on the large stale buffer, then a
    probe call that is smaller than the first and one with two operands and two results; the large call again.  Every result is
    bit for bit what the same call gives on a fresh handle."""
    big, _ = golden_args("rcp")
    sx, _ = golden_args("sincospi")
    ba, bb_ = golden_args("box_muller")
    calls = [
        lambda e: e.debug_math("rcp", big),
        lambda e: (e.normals(3, 1, 5, 16), None),
        lambda e: e.debug_math("rcp", big),
        lambda e: e.debug_math("sincospi", sx[:300]),
        lambda e: e.debug_math("box_muller", ba[:700], bb_[:700]),
        lambda e: (e.normals(3, 1, 5, 16), None),
        lambda e: e.debug_math("rcp", big),
    ]
    bits = lambda r: [None if v is None else v.tobytes() for v in r]
    with handle(lib) as e:
        got = [bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with handle(lib) as e:
            assert got[i] == bits(f(e)), i
    assert got[0] == got[2] == got[6]
