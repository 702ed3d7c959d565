"""Generates tests/golden/math_<fn>.npz: the arguments at which tests/_math_cases.py evaluates the functions of
barbay.jl_amd/csrc/bb_math.h (and the Box-Muller step of bb_block.h) through bb_debug_math, with their values from mpmath at 50
digits.  mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_math_golden.py [fn ...]        (all: under a minute)

Stored per file: the arguments `x` (and `y` where the function takes two) as float64 -- for box_muller the two 64-bit words as
uint64 -- and per output k the exact value as a float64 pair: `hi<k>`, the value rounded to a double, and `lo<k>`, the rest
(exact - hi) 2^shift rounded to a double, with `shift<k>` (int16) 0 except where |hi| < 2^-700: there it is 256, so that the rest
of a subnormal result, which no double holds, is stored as exactly as every other.  box_muller also stores the exact radius
sqrt(-2 ln u1) rounded to a double (`r`), the scale of its bound.

A function whose arguments do not fit one file of 75 KB (the largest golden committed before these) is cut into consecutive parts
math_<fn>.npz, math_<fn>_p1.npz, ...; `_math_cases.load` joins them.  The arguments are stored, not re-drawn by the tests: the
seeded draws below and the files' bytes (fixed zip time stamps) are reproducible, and arguments of the form exp(U) are rounded from
mpmath's exp, not libm's."""
import io
import math
import os
import struct
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
PART_BYTES = 75_000
LN2 = math.log(2.0)
TINY = 2.0 ** -700
FNS = ("exp", "exp_nonpos", "log", "log_1to2", "rcp", "div", "sqrt", "softplus_sigmoid", "sincospi", "box_muller")


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def _below(x):
    return np.nextafter(x, -np.inf)


def _above(x):
    return np.nextafter(x, np.inf)


def _exp_of(u):
    """exp(u) correctly rounded (mpmath), for arguments spread over the exponent range."""
    return np.array([float(mp.exp(mp.mpf(float(v)))) for v in u])


def _pow2(ks):
    return np.array([math.ldexp(1.0, int(k)) for k in ks])


def args_exp():
    g = np.random.default_rng(101)
    k = np.arange(-1070, 1024)
    return np.concatenate([
        np.linspace(-745.2, -707.0, 300), g.uniform(-745.2, -707.0, 200),            # subnormal results
        np.linspace(700.0, 709.78, 150), g.uniform(700.0, 709.78, 150),
        k * LN2, (k + 0.5) * LN2,                                                     # r = 0 and the largest |r|, every ldexp exponent
        [0.0, -0.0, 1e-300, -1e-300, 1e-17],
        g.uniform(-40.0, 40.0, 1000),
    ])


def args_exp_nonpos():
    x = args_exp()
    return x[x <= 0.0]


def args_log():
    g = np.random.default_rng(102)
    p2 = _pow2(np.arange(-1074, 1024))
    r = math.sqrt(0.5)
    fold = [r]
    for _ in range(4):
        fold = [_below(fold[0])] + fold + [_above(fold[-1])]
    fold = np.array(fold)
    return np.concatenate([
        p2, _below(p2[1:]),                                                           # (nothing positive lies below 2^-1074)
        fold, 2.0 * fold, 0.5 * fold, fold * 2.0 ** 300, fold * 2.0 ** -300,          # the mantissa fold at several exponents
        1.0 + np.arange(-20, 21) * 2.0 ** -52,
        1.0 + g.uniform(-1e-3, 1e-3, 400),
        _exp_of(g.uniform(-700.0, 700.0, 800)),
        [sys.float_info.max, 5e-324],
    ])


def args_log_1to2():
    g = np.random.default_rng(103)
    c = 2.0 * math.sqrt(0.5)
    fold = [c]
    for _ in range(4):
        fold = [_below(fold[0])] + fold + [_above(fold[-1])]
    return np.concatenate([
        np.array(fold), 1.0 + np.arange(1, 21) * 2.0 ** -52, 2.0 - np.arange(0, 21) * 2.0 ** -52,
        1.0 + np.array([2.0 ** -k for k in range(1, 53)]),                            # u = 1 + e for the e of softplus
        g.uniform(1.0, 2.0, 1000), 1.0 + _exp_of(g.uniform(-36.0, 0.0, 300)),
    ])


def _rcp_divisors(kmax):
    p2 = _pow2(np.arange(-kmax, kmax + 1))
    d = np.concatenate([p2, _below(p2)])
    return np.concatenate([d, -d])


def args_rcp():
    g = np.random.default_rng(104)
    sweep = np.concatenate([1.0 + np.arange(512) / 512.0, g.uniform(1.0, 2.0, 500), [_below(2.0), _above(1.0)]])
    rnd = _exp_of(g.uniform(-600.0, 600.0, 800)) * np.where(g.random(800) < 0.5, -1.0, 1.0)
    return np.concatenate([_rcp_divisors(1000), sweep, -sweep[:200], rnd])


def args_div():
    g = np.random.default_rng(105)
    b = np.concatenate([_rcp_divisors(500), 1.0 + np.arange(256) / 256.0, g.uniform(1.0, 2.0, 300),
                        _exp_of(g.uniform(-340.0, 340.0, 400)) * np.where(g.random(400) < 0.5, -1.0, 1.0)])
    a = g.standard_normal(b.size) * _exp_of(g.uniform(-20.0, 20.0, b.size))
    return np.concatenate([a, [0.0, -0.0]]), np.concatenate([b, [3.0, 3.0]])


def args_sqrt():
    g = np.random.default_rng(106)
    p4 = _pow2(2 * np.arange(-536, 512))                                              # 4^k: exact squares, normal with both neighbours
    return np.concatenate([
        _pow2(np.arange(-1074, 1024)), p4, _below(p4), _above(p4),
        g.uniform(1.0, 4.0, 800), np.arange(1, 41, dtype=np.float64) ** 2, _below(np.arange(2, 41, dtype=np.float64) ** 2),
        _exp_of(g.uniform(-600.0, 600.0, 800)),
        [5e-324, sys.float_info.max, 0.0],
        _exp_of(g.uniform(-744.0, -620.0, 300)),                                      # subnormal and tiny: the scaled branch (x < 2^-900)
        [2.0 ** -900, _below(2.0 ** -900), _above(2.0 ** -900), 2.0 ** -1022, _below(2.0 ** -1022), _above(2.0 ** -1022)],
    ])


def args_softplus_sigmoid():
    g = np.random.default_rng(107)
    return np.concatenate([
        np.linspace(-745.0, -700.0, 181), g.uniform(-745.0, -700.0, 100),
        np.arange(-800, 801) * 0.05,                                                  # -40 ... 40
        np.linspace(30.0, 800.0, 155), g.uniform(30.0, 800.0, 100),
        np.linspace(36.7, 37.5, 161), -np.linspace(36.7, 37.5, 161),                  # e crosses 2^-54 at |omega| = 37.43
        [0.0, -0.0],
        g.uniform(-8.0, 3.0, 800),
    ])


def args_sincospi():
    g = np.random.default_rng(108)
    m = np.arange(16) / 8.0                                                           # every multiple of 1/8 (and so of 1/4) in [0, 2)
    e = np.concatenate([m, _below(m[1:]), _above(m), [_below(2.0)]])
    return np.concatenate([e, [2.0 ** -k for k in range(0, 60)], g.uniform(0.0, 2.0, 1200), g.uniform(0.0, 0.25, 200)])


def args_box_muller():
    g = np.random.default_rng(109)
    lowbits = lambda n: g.integers(0, 2048, n, dtype=np.uint64)                       # the 11 bits the uniforms drop
    word = lambda m: (np.asarray(m, dtype=np.uint64) << np.uint64(11)) | lowbits(len(m))
    # u1 = (m + 1) 2^-53
    a_edge = word([0, 1, 2, 3, 2 ** 52 - 1, 2 ** 53 - 2, 2 ** 53 - 1])               # 2^-53, 2, 3, 4 x 2^-53, 1/2, 1 - 2^-53, 1
    a_tail = g.integers(0, 2 ** 20, 200, dtype=np.uint64)                            # u1 <= 2^-44: radius above 7.8
    a_rand = g.integers(0, 2 ** 64, 3000, dtype=np.uint64)
    # u2 = m 2^-53: the eight quadrant and octant boundaries of sincospi(2 u2), and one step to either side
    mb = np.array([(j * 2 ** 50 + d) % 2 ** 53 for j in range(8) for d in (-1, 0, 1)], dtype=np.uint64)
    b_edge = word(mb)
    a = np.concatenate([np.repeat(a_edge, b_edge.size), a_tail, a_rand])
    b = np.concatenate([np.tile(b_edge, a_edge.size), np.resize(b_edge, 100), g.integers(0, 2 ** 64, 100, dtype=np.uint64),
                        np.resize(b_edge, 240), g.integers(0, 2 ** 64, 2760, dtype=np.uint64)])
    return a, b


# ---- 50-digit values ---------------------------------------------------------------------------------------------------------
def _softplus(x):
    return x + mp.log1p(mp.exp(-x)) if x > 0 else mp.log1p(mp.exp(x))


def _sigmoid(x):
    return 1 / (1 + mp.exp(-x)) if x > 0 else mp.exp(x) / (1 + mp.exp(x))


def _box_muller(a, b):
    u1 = mp.mpf((int(a) >> 11) + 1) / 2 ** 53
    u2 = mp.mpf(int(b) >> 11) / 2 ** 53
    r = mp.sqrt(-2 * mp.log(u1))
    return r * mp.cospi(2 * u2), r * mp.sinpi(2 * u2), r


EXACT = {
    "exp": lambda x: (mp.exp(x),),
    "exp_nonpos": lambda x: (mp.exp(x),),
    "log": lambda x: (mp.log(x),),
    "log_1to2": lambda x: (mp.log(x),),
    "rcp": lambda x: (1 / x,),
    "div": lambda x, y: (x / y,),
    "sqrt": lambda x: (mp.sqrt(x),),
    "softplus_sigmoid": lambda x: (_softplus(x), _sigmoid(x)),
    "sincospi": lambda x: (mp.sinpi(x), mp.cospi(x)),
}
ARGS = {"exp": args_exp, "exp_nonpos": args_exp_nonpos, "log": args_log, "log_1to2": args_log_1to2, "rcp": args_rcp, "div": args_div,
        "sqrt": args_sqrt, "softplus_sigmoid": args_softplus_sigmoid, "sincospi": args_sincospi, "box_muller": args_box_muller}


def _to_double(v):
    """v rounded to the nearest double, subnormals included (one rounding: through an exact integer ratio)."""
    if v == 0:
        return 0.0
    s = -1.0 if v < 0 else 1.0
    v = abs(v)
    e = max(mp.frexp(v)[1] - 53, -1074)                                               # the ulp of the result: v = m 2^ex, m in [1/2, 1)
    n = int(mp.nint(v / mp.mpf(2) ** e))                                              # <= 2^53 (nint: to nearest, ties to even)
    return s * math.ldexp(float(n), e)


def split(v):
    hi = _to_double(v)
    shift = 256 if abs(hi) < TINY else 0
    return hi, float((v - mp.mpf(hi)) * mp.mpf(2) ** shift), shift


def table(fn):
    a = ARGS[fn]()
    if fn == "box_muller":
        wa, wb = a
        vals = [_box_muller(p, q) for p, q in zip(wa, wb)]
        d = {"x": wa, "y": wb, "r": np.array([_to_double(v[2]) for v in vals])}
        vals = [v[:2] for v in vals]
    elif fn == "div":
        x, y = (np.asarray(v, dtype=np.float64) for v in a)
        vals = [EXACT[fn](mp.mpf(float(p)), mp.mpf(float(q))) for p, q in zip(x, y)]
        d = {"x": x, "y": y}
    else:
        x = np.asarray(a, dtype=np.float64)
        vals = [EXACT[fn](mp.mpf(float(p))) for p in x]
        d = {"x": x}
    for k in range(len(vals[0])):
        parts = [split(v[k]) for v in vals]
        d[f"hi{k}"] = np.array([p[0] for p in parts])
        d[f"lo{k}"] = np.array([p[1] for p in parts])
        d[f"shift{k}"] = np.array([p[2] for p in parts], dtype=np.int16)
    return d


# ---- files -------------------------------------------------------------------------------------------------------------------
def npz_bytes(arrays):
    """An .npz as numpy.load reads it, with fixed time stamps: equal arrays give equal bytes."""
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zi, b.getvalue())
    return out.getvalue()


def part_path(fn, p):
    return os.path.join(HERE, f"math_{fn}.npz" if p == 0 else f"math_{fn}_p{p}.npz")


def write(fn):
    d = table(fn)
    n = len(d["x"])
    nparts = 1
    while True:                                                                       # the fewest equal parts that all fit
        cuts = [n * p // nparts for p in range(nparts + 1)]
        blobs = [npz_bytes({k: v[cuts[p]:cuts[p + 1]] for k, v in d.items()}) for p in range(nparts)]
        if max(len(b) for b in blobs) <= PART_BYTES:
            break
        nparts += 1
    p = 0
    while os.path.exists(part_path(fn, p)):                                           # (parts of an earlier, longer table)
        os.remove(part_path(fn, p))
        p += 1
    for p, b in enumerate(blobs):
        with open(part_path(fn, p), "wb") as f:
            f.write(b)
    return n, [len(b) for b in blobs]


def main(argv):
    for fn in argv or FNS:
        n, sizes = write(fn)
        print(f"{fn:18s} {n:5d} arguments, {len(sizes)} file(s): {sizes} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
