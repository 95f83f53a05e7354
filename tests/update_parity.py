"""Element-wise float64 parity bound for the six fused kernels of the PPO minibatch update (cadre_amd/csrc/ppo_update.hip) — the bound,
stated once ("update parity").  Same ruler as tests/f32_parity.py: every stored output element is pinned to

    |got - y64|  <=  c_bar * 2^-24 * mag

against float64 of the operands AS STORED, stage by stage: every kernel here stores its intermediates, so each stored output is
compared with float64 of the stored inputs of its stage, and nothing is chained through two stages except where the kernel itself keeps
a value in registers (the pre-activation of the forward step, dh and dct of the backward step).  `mag` is the reference on absolute values,
`c_bar` comes from f32_parity.c_bar_direct on the case's own products (strictly sequential fp32 chain, every output, doubled) and is
asserted under DIRECT_CAP(K) = K + 5.  An output whose magnitude is zero (an empty run, a padding column, a ReLU-masked gradient, a gate
that is exactly 0) has no unit: it must be an exact zero.  Every checked output is finite.  No sampling, no exempt share.

cadre_lstm_step_fwd.  pre64 = Gx + h W^T + b (K = D products, Gx and b as residual and shift), delta = c_bar 2^-24 mag; the chain of c_bar
starts from Gx + b, as the kernel's accumulator does (`direct`, seed_first: with the residual added behind the sum, a sequential fp32
evaluation in the kernel's own order left its enclosure by 17 ulps where Gx = -43 dwarfs the products — the bound was wrong, not the order).  The pre-activation
is not stored; sigmoid and tanh are monotone, so the stored gate must lie in the ENCLOSURE [act64(pre64 - delta), act64(pre64 + delta)],
widened by T ulps of the larger endpoint (one ulp := 2^-23 |v|) and by the absolute floor 2^-126 (where expf overflows the kernel gives 0,
float64 a number below the smallest normal fp32).  c_t against float64 of fg c_prev + ig gg on the STORED fp32 gates, ruler
|fg||c_prev| + |ig||gg|, bar CT_BAR = 3 units: the kernel forms fma(fg, c_prev, RN(ig gg)) — the term ig gg meets two roundings (its own
product and the final one), the term fg c_prev one (two without the contraction), each rounding at most 2^-24 of a value that the ruler
bounds — so at most 2 (1 + 2^-24) units in any order, and one unit is spare.  tanh(c_t) against tanh64 of the stored c_t within T_TANH ulps
plus the floor.  h_t is one fp32 product of two stored values: bit-identical to np.float32(og) * np.float32(tc).

cadre_lstm_step_bwd.  dh64 = dG_t W + dh_in (K = 4 D), mag_dh = sum|dG||W| + |dh_in|, c_bar_dh from the sequential chain.  The cell backward
is a polynomial in dh and the stored gates, tanh c, c_prev, dc (cell_bwd below, the kernel's own expression); it is evaluated in float64 on
(value, magnitude) pairs (class VM: magnitudes add under + and -, multiply under *, the constant 1 has magnitude 1, mag_dh stands in for
|dh|).  Every output is linear in dh, so the product's error reaches it multiplied by exactly the factors that multiply mag_dh inside mag_out:

    |got - out64|  <=  (c_bar_dh + c_poly) * 2^-24 * mag_out.

c_poly = FACTOR x the worst error, in units of mag_out, of an fp32 numpy evaluation of the polynomial on dh rounded to fp32, over four
association orders (products left to right as written / right to left, each with and without contracting dc + (..)(..) and 1 - x x into
fmas).  It is asserted under N_POLY = 7, the longest chain of roundings from an input to an output:  tc -> tc tc (1) -> 1 - . (2) ->
(dh og) . (3) -> dc + . (4) = dct -> dct gg (5) -> . ig (6) -> . (1 - ig) (7); from dh the same count (its own rounding to fp32, dh og, the
product with 1 - tc tc, the sum, three products); the f gate has the same seven, the g gate six, the o gate three (four with dh's), dc five.
Per term of mag_out that is a factor (1 + d)^7 - 1 <= 7.000003 x 2^-24.  with_product = 0: dh is dh_in exactly and c_bar_dh = 0 — the tight case.

cadre_lstm_dw.  dW_hh, dW_ih: direct products over K = S x (rows of the net's run); db the product with a column of ones (mag = sum|dG|):
the ones ride as one more column of the second operand, so a case has ONE c_bar over all its outputs.  An empty run: exact zeros.

cadre_mlp_fwd.  A1 = relu(H W1^T + b1), K = D; A2 from the STORED A1, K = 128; O3 from the stored A2, K = 128 (epilogue32, act = 1 / 0).
cadre_mlp_bwd.  dA2 = (dO3 W3) where stored A2 > 0, K = 64; dA1 = (stored dA2 W2) where stored A1 > 0, K = 128; dH = the two towers of a net in
ONE accumulation, K = 256.  A masked element has magnitude zero: exact zero.
cadre_mlp_dw.  Six gradients per tower, direct over K = rows of the run, from the stored dO3, dA2, dA1, A2, A1, H.

T_EXP = 3, T_TANH = 5 ulps: the OpenCL full-profile limits of single-precision exp and tanh, which the device math library (OCML) is built
to.  No accuracy table of the library's own is in the ROCm tree used for development (documentation, OCML and HIP headers searched; the one
ulp figure in the compiler's OpenCL header concerns fast_normalize), and no text of the OpenCL specification either: the two figures are the
specification's as remembered and are NOT taken from the kernels' output.  T_ACT = T_EXP + 2 for sigmoid_(x) = 1 / (1 + expf(-x)): the add and
the correctly rounded divide cost at most one ulp each (d/de of 1 / (1 + e) is at most 1 in relative terms).  The GPU tests print the worst
OBSERVED ulp distances next to these; an observed value is recorded, never used as the bar.

Plain helper module (no GPU, no fixtures).  The fp32 numpy emulations at the end (strictly sequential, and in the kernels' own shape) and
their mutants serve tests/test_update_parity_cpu.py; tests/test_update_parity_gpu.py applies the bound to the kernels."""
import numpy as np
import torch

from tests import bf16_parity as bp
from tests import f32_parity as fp  # noqa: F401
from tests.bf16_parity import U, f64, dense_acc, dense_products
from tests.f32_parity import FACTOR, DIRECT_CAP, DIRECT_BUDGET, c_bar_direct, chain_outputs, check32, epilogue32, trunc_mantissa  # noqa: F401

T_EXP, T_TANH = 3.0, 5.0
T_ACT = T_EXP + 2.0
ULP = 2.0 ** -23          # one ulp of v := ULP * |v|
FLOOR = 2.0 ** -126       # smallest normal fp32
CT_BAR = 3.0
N_POLY = 7
F4, F8 = np.float32, np.float64


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _flat(t):
    return np.asarray(f64(t)).reshape(-1)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F4))


# ----------------------------------------------------------------------------- float64 transcendentals
def sig64(x):
    x = np.asarray(x, dtype=F8)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def tanh64(x):
    return np.tanh(np.asarray(x, dtype=F8))


# ----------------------------------------------------------------------------- (value, magnitude) pairs
class VM:
    """A float64 value with the magnitude of the expression that formed it."""

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=F8)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=F8)

    @staticmethod
    def of(x):
        return x if isinstance(x, VM) else VM(x)

    def __add__(self, o):
        o = VM.of(o)
        return VM(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        o = VM.of(o)
        return VM(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        o = VM.of(o)
        return VM(o.v - self.v, o.m + self.m)

    def __mul__(self, o):
        o = VM.of(o)
        return VM(self.v * o.v, self.m * o.m)

    __radd__, __rmul__ = __add__, __mul__


def cell_bwd(dh, dc, ig, fg, gg, og, tc, cp):
    """The cell backward as lstm_step_bwd_kernel writes it -> [dG_i, dG_f, dG_g, dG_o, dc_prev]; generic over the operand type (VM,
    float64 arrays, torch tensors)."""
    dct = dc + dh * og * (1.0 - tc * tc)
    return [dct * gg * ig * (1.0 - ig), dct * cp * fg * (1.0 - fg), dct * ig * (1.0 - gg * gg), dh * tc * og * (1.0 - og), dct * fg]


def _fma(a, b, c):
    return (a.astype(F8) * b.astype(F8) + c.astype(F8)).astype(F4)


def cell_bwd32(dh, dc, ig, fg, gg, og, tc, cp, right=False, fma=False, cp_f=None, lin_tc=False):
    """cell_bwd in fp32 numpy.  right: products associated right to left; fma: dc + (..)(..) and 1 - x x contracted.  Mutants: cp_f stands in
    for c_prev in the f gate's gradient; lin_tc: (1 - tc) for (1 - tc tc)."""
    one = F4(1)
    assert all(a.dtype == F4 for a in (dh, dc, ig, fg, gg, og, tc, cp))
    om = lambda x: _fma(-x, x, np.full_like(x, one)) if fma else one - x * x
    omt = one - tc if lin_tc else om(tc)
    omg = om(gg)
    a, b = (dh, og * omt) if right else (dh * og, omt)
    dct = _fma(a, b, dc) if fma else dc + a * b
    m4 = (lambda w, x, y, z: w * (x * (y * z))) if right else (lambda w, x, y, z: ((w * x) * y) * z)
    cf = cp if cp_f is None else cp_f
    out = [m4(dct, gg, ig, one - ig), m4(dct, cf, fg, one - fg), dct * (ig * omg) if right else (dct * ig) * omg, m4(dh, tc, og, one - og), dct * fg]
    assert all(o.dtype == F4 for o in out)
    return out


POLY_ORDERS = [(right, fma) for right in (False, True) for fma in (False, True)]


# ----------------------------------------------------------------------------- one direct stage
def direct(A, Bm, shift=None, resid=None, act=0, what="", seed_first=False):
    """A [M][K] . Bm [N][K]^T (+ shift over the columns, + resid, ReLU when act = 1) -> (y64, mag, c_bar or None, cap): the float64 reference,
    its magnitude, and c_bar_direct over EVERY output whose magnitude is not zero (None when there is none).  seed_first: the chain starts
    from resid + shift and adds the products to it (two more terms in front of the K products, cap DIRECT_CAP(K + 2)) instead of adding them
    behind the sum — the forward step's order (its accumulator is seeded with Gx + b), and the less favourable one where |Gx| is large
    against the products: every one of the K additions then rounds at the seed's magnitude, not only the last."""
    A, Bm = A.contiguous(), Bm.contiguous()
    K = A.shape[1]
    assert A.shape[0] * Bm.shape[0] * K <= DIRECT_BUDGET, "%s: choose a shape whose every chain can be summed" % what
    acc, mac = dense_acc(A, Bm)
    y, mag = epilogue32(acc, mac, None, shift, resid, act)
    live = np.flatnonzero(mag.reshape(-1).numpy() > 0).astype(np.int64)
    if live.size == 0:
        return y, mag, None, DIRECT_CAP(K)
    if seed_first:
        assert act == 0 and shift is not None and resid is not None
        rn, sn, N = _np(resid).astype(F4).reshape(-1), _np(shift).astype(F4).reshape(-1), Bm.shape[0]
        seed = (lambda idx: np.stack([rn[idx], sn[idx % N]], 1), 2, rn.size)
        cb, cap = c_bar_direct([seed, dense_products(A, Bm)], y, mag, what=what, idx=live)
    else:
        cb, cap = c_bar_direct([dense_products(A, Bm)], y, mag, None, shift, resid, act, what=what, idx=live)
    return y, mag, cb, cap


# ----------------------------------------------------------------------------- the collector of one test case
class Case:
    """The pieces (one per net / tower) of one test case; finish() checks every element of every piece — one c_bar per output kind, the
    largest over the pieces, which is c_bar_direct over all outputs of the case — and prints one line per output kind."""

    def __init__(self, what):
        self.what, self.units, self.encl, self.bits, self.stats = what, {}, {}, {}, {}

    def add_units(self, name, got, y, mag, cb, cap):
        assert tuple(got.shape) == tuple(y.shape) == tuple(mag.shape), "%s %s: shape %s vs %s" % (self.what, name, tuple(got.shape), tuple(y.shape))
        self.units.setdefault(name, []).append((_flat(got), _flat(y), _flat(mag), cb, cap))

    def add_enclosure(self, name, got, lo, hi, T, exact=None, centre=None):
        n = _flat(got).size
        ex = np.zeros(n, bool) if exact is None else np.asarray(exact).reshape(-1)
        ce = np.zeros(n) if centre is None else _flat(centre)
        self.encl.setdefault(name, []).append((_flat(got), _flat(lo), _flat(hi), T, ex, ce))

    def add_bits(self, name, got, want):
        self.bits.setdefault(name, []).append((np.ascontiguousarray(_np(got), dtype=F4).reshape(-1), np.ascontiguousarray(_np(want), dtype=F4).reshape(-1)))

    def finish(self):
        for name, parts in self.units.items():
            tag = "%s %s" % (self.what, name)
            g, y, m = (np.concatenate([p[i] for p in parts]) for i in range(3))
            cbs, cap = [p[3] for p in parts if p[3] is not None], max(p[4] for p in parts)
            assert np.isfinite(g).all(), "%s: non-finite output" % tag
            dead = m == 0
            assert not np.any(y[dead]), "%s: the helper is wrong (a reference without magnitude is not zero)" % tag
            assert not np.any(g[dead]), "%s: %d of %d outputs whose magnitude is zero are no exact zeros" % (tag, int(np.count_nonzero(g[dead])), int(dead.sum()))
            if dead.all():
                print("%s: %d elements, all exact zeros" % (tag, g.size))
                continue
            assert cbs, "%s: the helper is wrong (live outputs without a c_bar)" % tag
            live = ~dead
            st = check32(torch.from_numpy(g[live]), torch.from_numpy(y[live]), torch.from_numpy(m[live]), max(cbs), cap,
                         what="%s (+ %d exact zeros)" % (tag, int(dead.sum())))
            self.stats[name] = (st["excess"], st["c_bar"], cap)
        for name, parts in self.encl.items():
            tag = "%s %s" % (self.what, name)
            g, lo, hi = (np.concatenate([p[i] for p in parts]) for i in range(3))
            T = parts[0][3]
            exact, centre = np.concatenate([p[4] for p in parts]), np.concatenate([p[5] for p in parts])
            assert np.isfinite(g).all(), "%s: non-finite output" % tag
            lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
            vmax = np.maximum(np.abs(lo), np.abs(hi))
            over = np.maximum(np.maximum(np.maximum(lo - g, g - hi), 0.0) - FLOOR, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                ex = np.where(over > 0, over / (ULP * vmax), 0.0)
            worst = int(np.argmax(ex))
            sel = exact & (np.abs(centre) >= FLOOR)
            obs = float(np.max(np.abs(g[sel] - centre[sel]) / (ULP * np.abs(centre[sel])))) if sel.any() else float("nan")
            print("%s: outside its enclosure by %.3f ulp <= T %.0f; observed %.3f ulp at the %d arguments known exactly; %d elements"
                  % (tag, ex[worst], T, obs, int(sel.sum()), g.size))
            self.stats[name] = (float(ex[worst]), T, obs)
            assert ex[worst] <= T, ("%s: element %d outside its enclosure by %.3f ulp > T %.0f: got %.9g, enclosure [%.9g, %.9g]"
                                    % (tag, worst, ex[worst], T, g[worst], lo[worst], hi[worst]))
        for name, parts in self.bits.items():
            g, w = (np.concatenate([p[i] for p in parts]) for i in range(2))
            bad = g.view(np.uint32) != w.view(np.uint32)
            print("%s %s: %d elements, %d not bit-identical" % (self.what, name, g.size, int(bad.sum())))
            assert not bad.any(), "%s %s: %d of %d elements not bit-identical (first at %d: got %.9g, want %.9g)" % (
                self.what, name, int(bad.sum()), g.size, int(np.argmax(bad)), g[np.argmax(bad)], w[np.argmax(bad)])
        return self.stats


# ----------------------------------------------------------------------------- the bound, per kernel (rows = one net's run)
def lstm_fwd_check(case, W, b, Gx, hp, cp, got):
    """W [4D][D], b [4D], Gx [n][4D], hp / cp [n][D] as stored (fp32 tensors); got: act [n][4D], c / tc / h [n][D] as the kernel stored them."""
    D = hp.shape[1]
    pre, mag, cb, cap = direct(hp, W, shift=b, resid=Gx, what=case.what + " pre-activation", seed_first=True)
    case.pre_cb = max(getattr(case, "pre_cb", 0.0), cb or 0.0)
    pre, mag = pre.numpy(), mag.numpy()
    delta = (cb or 0.0) * U * mag
    exact = mag == np.abs(_np(Gx).astype(F8))                # no product, no bias: the kernel's pre-activation is Gx itself
    for name, fn, T, cols in (("sigmoid gates", sig64, T_ACT, np.r_[0:2 * D, 3 * D:4 * D]), ("tanh gate", tanh64, T_TANH, np.r_[2 * D:3 * D])):
        case.add_enclosure(name, _np(got["act"])[:, cols], fn(pre[:, cols] - delta[:, cols]), fn(pre[:, cols] + delta[:, cols]), T,
                           exact[:, cols], fn(pre[:, cols]))
    ig, fg, gg, og = (f64(t).numpy() for t in got["act"].view(-1, 4, D).unbind(1))
    c0 = f64(cp).numpy()
    case.add_units("c_t", got["c"], t64(fg * c0 + ig * gg), t64(np.abs(fg * c0) + np.abs(ig * gg)), CT_BAR, int(CT_BAR))
    tc = tanh64(f64(got["c"]).numpy())
    case.add_enclosure("tanh(c_t)", got["tc"], tc, tc, T_TANH, np.ones(tc.shape, bool), tc)
    case.add_bits("h_t", got["h"], _np(got["act"][:, 3 * D:]).astype(F4) * _np(got["tc"]).astype(F4))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F8))


def lstm_bwd_check(case, W, dG_t, dh_in, act, tc, cp, dc, got_dG, got_dC, with_product):
    """W [4D][D]; dG_t [n][4D]; dh_in, tc, cp, dc [n][D]; act [n][4D] as stored; got_dG [n][4D], got_dC [n][D] — the rows the net owns."""
    D = tc.shape[1]
    if with_product:
        dh, mag_dh, cb_dh, cap_dh = direct(dG_t, W.t(), resid=dh_in, what=case.what + " dh")
        dh, mag_dh, cb_dh = dh.numpy(), mag_dh.numpy(), cb_dh or 0.0
    else:
        dh, cb_dh, cap_dh = f64(dh_in).numpy(), 0.0, 0
        mag_dh = np.abs(dh)
    ops = [f64(dc).numpy()] + [f64(t).numpy() for t in act.view(-1, 4, D).unbind(1)] + [f64(tc).numpy(), f64(cp).numpy()]
    outs = cell_bwd(VM(dh, mag_dh), *[VM(o) for o in ops])
    y, mag = np.concatenate([o.v for o in outs], 1), np.concatenate([o.m for o in outs], 1)
    ops32 = [dh.astype(F4)] + [o.astype(F4) for o in ops]
    live = mag > 0
    worst = 0.0
    for right, fma in POLY_ORDERS:
        e = np.abs(np.concatenate(cell_bwd32(*ops32, right=right, fma=fma), 1).astype(F8) - y)
        worst = max(worst, float((e[live] / (U * mag[live])).max()))
    c_poly = FACTOR * worst
    assert 0 < c_poly <= N_POLY, "%s: c_poly %.3g outside (0, N_POLY = %d]: the helper is wrong" % (case.what, c_poly, N_POLY)
    case.c_poly, case.cb_dh = max(getattr(case, "c_poly", 0.0), c_poly), max(getattr(case, "cb_dh", 0.0), cb_dh)
    case.add_units("dG, dc", torch.cat([got_dG, got_dC], 1), t64(y), t64(mag), cb_dh + c_poly, cap_dh + N_POLY)


def dw_check(case, name, dY, Ys, got_w, got_b):
    """dY [K][M] (gate / layer gradients of the run's rows), Ys: list of [K][N_i] second operands; got_w: list of [M][N_i]; got_b [M] (the
    column sums) — one accumulation per output, the ones column with the rest."""
    K, M = dY.shape
    if K == 0:
        for w in got_w:
            case.add_units(name, w, torch.zeros(w.shape, dtype=torch.float64), torch.zeros(w.shape, dtype=torch.float64), None, DIRECT_CAP(0))
        case.add_units(name, got_b, torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64), None, DIRECT_CAP(0))
        return
    Y = torch.cat(list(Ys) + [torch.ones(K, 1)], 1)
    y, mag, cb, cap = direct(dY.t(), Y.t(), what="%s %s" % (case.what, name))
    got = torch.cat(list(got_w) + [got_b.reshape(M, 1)], 1)
    case.add_units(name, got, y, mag, cb, cap)


def mlp_fwd_check(case, H, P, got):
    """H [n][D]; P = (W1 [128][D], b1, W2, b2, W3 [64][128], b3); got: A1, A2 [n][128], O3 [n][64] as stored."""
    W1, b1, W2, b2, W3, b3 = P
    for name, X, W, b, act in (("A1", H, W1, b1, 1), ("A2", got["A1"], W2, b2, 1), ("O3", got["A2"], W3, b3, 0)):
        y, mag, cb, cap = direct(X, W, shift=b, act=act, what="%s %s" % (case.what, name))
        case.add_units(name, got[name], y, mag, cb, cap)


def mlp_bwd_check(case, dO3, A1, A2, P0, P1, got):
    """One net: dO3 [2][n][64], stored A1 / A2 [2][n][128], the two towers' parameters; got: dA2, dA1 [2][n][128], dH [n][D]."""
    for tw, P in enumerate((P0, P1)):
        y, mag, cb, cap = direct(dO3[tw], P[4].t(), what=case.what + " dA2")
        keep = f64(A2[tw] > 0)
        case.add_units("dA2", got["dA2"][tw], y * keep, mag * keep, cb, cap)
        y, mag, cb, cap = direct(got["dA2"][tw], P[2].t(), what=case.what + " dA1")
        keep = f64(A1[tw] > 0)
        case.add_units("dA1", got["dA1"][tw], y * keep, mag * keep, cb, cap)
    y, mag, cb, cap = direct(torch.cat([got["dA1"][0], got["dA1"][1]], 1), torch.cat([P0[0].t(), P1[0].t()], 1), what=case.what + " dH")
    case.add_units("dH", got["dH"], y, mag, cb, cap)


def mlp_dw_check(case, dO3, dA2, dA1, A2, A1, H, got):
    """One tower on its run's rows; got = (dW1 [128][D], db1, dW2, db2, dW3 [64][128], db3)."""
    dw_check(case, "dW1, db1", dA1, [H], [got[0]], got[1])
    dw_check(case, "dW2, db2", dA2, [A1], [got[2]], got[3])
    dw_check(case, "dW3, db3", dO3, [A2], [got[4]], got[5])


# ----------------------------------------------------------------------------- test data
def saturating(r, shape, sd=0.7, tenth=15.0):
    """Pre-activation-like fp32 values: N(0, sd), a tenth of them N(0, tenth) instead (|x| to 30 and beyond: saturated gates)."""
    x = r.standard_normal(shape) * sd
    wide = r.random_sample(shape) < 0.1
    return np.where(wide, r.standard_normal(shape) * tenth, x).astype(F4)


def log_uniform(r, shape, lo, hi):
    """+-10^uniform(lo, hi), fp32."""
    return (10.0 ** r.uniform(lo, hi, shape) * r.choice([-1.0, 1.0], shape)).astype(F4)


SPECIALS = np.array([100.0, -100.0, 0.0, -0.0, 100.0, -100.0, 0.0, 1e-3, -1e-3, 30.0, -30.0, 1e-6], dtype=F4)


def lstm_fwd_operands(r, Z, B, D, saturate):
    """Stored operands of one forward step, un-padded: W [Z][4D][D], b [Z][4D], Gx [Z][B][4D], hp, cp [Z][B][D] (fp32 tensors).  saturate:
    Gx from `saturating` (pre-activations to +-30 in a tenth of the elements), c_prev log-uniform so that |c_t| spans 1e-4 .. 20, and two
    units per net (3 and D - 1) WITHOUT weights and bias, whose pre-activation is Gx exactly: there Gx cycles through SPECIALS
    (+-100, +-0, +-30, small), a few dozen elements per net."""
    W = r.standard_normal((Z, 4 * D, D)).astype(F4) * F4(0.04 if D > 100 else 0.15)
    b = r.standard_normal((Z, 4 * D)).astype(F4) * F4(0.1)
    hp = r.standard_normal((Z, B, D)).astype(F4) * F4(0.5)
    if not saturate:
        Gx, cp = r.standard_normal((Z, B, 4 * D)).astype(F4) * F4(0.5), r.standard_normal((Z, B, D)).astype(F4)
    else:
        Gx, cp = saturating(r, (Z, B, 4 * D)), log_uniform(r, (Z, B, D), -4, 1.3)
        for u in (3, D - 1):
            for g in range(4):
                W[:, g * D + u] = 0
                b[:, g * D + u] = 0
                Gx[:, :, g * D + u] = SPECIALS[(np.arange(B)[None] + 3 * g + np.arange(Z)[:, None] + u) % len(SPECIALS)]
    return tuple(torch.from_numpy(a) for a in (W, b, Gx, hp, cp))


def lstm_bwd_operands(r, Z, B, D, saturate):
    """Stored operands of one backward step: dG_t [Z][B][4D], dh_in, dc, cp, tc [Z][B][D], act [Z][B][4D] (fp32 tensors).  saturate: the
    gates and tanh c are np.float32 of float64 sigmoid / tanh of `saturating` values — gates of exactly 1.0f and tc of +-1.0f occur."""
    pre = saturating(r, (Z, B, 4 * D)) if saturate else r.standard_normal((Z, B, 4 * D)).astype(F4)
    act = np.concatenate([sig64(pre[..., :2 * D]), tanh64(pre[..., 2 * D:3 * D]), sig64(pre[..., 3 * D:])], -1).astype(F4)
    cp = log_uniform(r, (Z, B, D), -4, 1.3) if saturate else r.standard_normal((Z, B, D)).astype(F4)
    c = (act[..., D:2 * D] * cp + act[..., :D] * act[..., 2 * D:3 * D]).astype(F4)
    tc = tanh64(c).astype(F4)
    dG_t, dh_in, dc = (r.standard_normal(s).astype(F4) * F4(0.3) for s in ((Z, B, 4 * D), (Z, B, D), (Z, B, D)))
    if saturate:
        assert (act[..., :2 * D] == 1).any() and (np.abs(tc) == 1).any(), "choose a seed with a gate of 1.0f and a tanh c of +-1.0f"
    return tuple(torch.from_numpy(a) for a in (dG_t, dh_in, dc, cp, tc, act))


def runs_own(runs, B):
    """[(first, count)] per net -> bool [Z][B]."""
    own = torch.zeros(len(runs), B, dtype=torch.bool)
    for z, (lo, n) in enumerate(runs):
        own[z, lo:min(B, lo + n)] = True
    return own


# ----------------------------------------------------------------------------- fp32 numpy emulations of the kernels' arithmetic
def dot32(A, Bm, order="seq", seed=None, quarters=1):
    """A [M][K] . Bm [N][K]^T in fp32 numpy, products rounded to fp32.  seq: strictly sequential from `seed` (or 0).  kernel: the kernels' own
    shape — partial sums of 4 along K (one v_mfma_f32_16x16x4_f32 each), alternately added to two accumulators (the first starts from
    `seed`) that are added at the end; quarters = 4: K cut in four contiguous quarters summed so, added as (q0 + q1) + (q2 + q3)."""
    a, b = np.ascontiguousarray(_np(A), dtype=F4), np.ascontiguousarray(_np(Bm), dtype=F4)
    P = a[:, None, :] * b[None, :, :]
    sd = None if seed is None else np.ascontiguousarray(_np(seed), dtype=F4)
    if order == "seq":
        if sd is not None:
            P = np.concatenate([sd[..., None], P], -1)
        return np.cumsum(P, -1, dtype=F4)[..., -1]
    assert order == "kernel" and (sd is None or quarters == 1)
    pad = -P.shape[-1] % (8 * quarters)
    if pad:
        P = np.concatenate([P, np.zeros(P.shape[:-1] + (pad,), F4)], -1)
    s4 = np.cumsum(P.reshape(P.shape[:2] + (quarters, -1, 4)), -1, dtype=F4)[..., -1]
    acc = []
    for qd in range(quarters):
        e, o = s4[:, :, qd, 0::2], s4[:, :, qd, 1::2]
        if sd is not None:
            e = np.concatenate([sd[..., None], e], -1)
        acc.append(np.cumsum(e, -1, dtype=F4)[..., -1] + np.cumsum(o, -1, dtype=F4)[..., -1])
    return (acc[0] + acc[1]) + (acc[2] + acc[3]) if quarters == 4 else acc[0]


def sig32(x):
    return sig64(x).astype(F4)


def tanh32(x):
    return tanh64(x).astype(F4)


def tanh_by_sigmoid32(x):
    """Mutant: tanh x = 2 sigmoid(2x) - 1 in fp32 (cancels around 0)."""
    return F4(2) * sig32(F4(2) * x) - F4(1)


def sig_rough_exp32(x):
    """Mutant: 1 / (1 + e) in fp32 with an e = exp(-x) that is 2^-18 too large."""
    with np.errstate(over="ignore"):
        e = (np.exp(-x.astype(F8)) * (1 + 2.0 ** -18)).astype(F4)
        return F4(1) / (F4(1) + e)


def lstm_fwd_emulate(W, b, Gx, hp, cp, order="seq", sig=sig32, tanh=tanh32, bias_gates=4, quant=None):
    """The forward step of one net in fp32 numpy -> dict(act, c, tc, h) of fp32 tensors.  Mutants: sig / tanh, the bias on the first
    `bias_gates` gates only, quant applied to both operands of the product."""
    D = hp.shape[1]
    bb = _np(b).astype(F4).copy()
    bb[bias_gates * D:] = 0
    A, Wm = (quant(hp), quant(W)) if quant else (hp, W)
    pre = dot32(A, Wm, order, _np(Gx).astype(F4) + bb[None])
    ig, fg, gg, og = sig(pre[:, :D]), sig(pre[:, D:2 * D]), tanh(pre[:, 2 * D:3 * D]), sig(pre[:, 3 * D:])
    c = _fma(fg, _np(cp).astype(F4), ig * gg)
    tc = tanh(c)
    return dict(act=t32(np.concatenate([ig, fg, gg, og], 1)), c=t32(c), tc=t32(tc), h=t32(og * tc))


def lstm_bwd_emulate(W, dG_t, dh_in, act, tc, cp, dc, with_product, order="seq", right=False, fma=False, cp_f=None, lin_tc=False, quant=None):
    """The backward step of one net in fp32 numpy -> (dG [n][4D], dc_prev [n][D]) fp32 tensors."""
    D = tc.shape[1]
    dh = _np(dh_in).astype(F4)
    if with_product:
        A, Wm = (quant(dG_t), quant(W)) if quant else (dG_t, W)
        dh = dot32(A, Wm.t(), "seq", dh) if order == "seq" else dh + dot32(A, Wm.t(), "kernel", None, 4)
    gates = [_np(t).astype(F4) for t in act.view(-1, 4, D).unbind(1)]
    out = cell_bwd32(dh, _np(dc).astype(F4), *gates, _np(tc).astype(F4), _np(cp).astype(F4), right=right, fma=fma,
                     cp_f=None if cp_f is None else _np(cp_f).astype(F4), lin_tc=lin_tc)
    return t32(np.concatenate(out[:4], 1)), t32(out[4])


def dw_emulate(dY, Ys, order="seq", quant=None):
    """dY [K][M], Ys list of [K][N_i] -> ([dW_i [M][N_i]], db [M]) fp32 tensors."""
    q = quant or (lambda t: t)
    M = dY.shape[1]
    if dY.shape[0] == 0:
        return [torch.zeros(M, Y.shape[1]) for Y in Ys], torch.zeros(M)
    return [t32(dot32(q(dY).t(), q(Y).t(), order)) for Y in Ys], t32(dot32(dY.t(), torch.ones(1, dY.shape[0]), order)[:, 0])


def mlp_fwd_emulate(H, P, order="seq", quant=None):
    q = quant or (lambda t: t)
    W1, b1, W2, b2, W3, b3 = P
    lin = lambda X, W, b: dot32(q(X), q(W), order) + _np(b).astype(F4)[None]
    A1 = t32(np.maximum(lin(H, W1, b1), F4(0)))
    A2 = t32(np.maximum(lin(A1, W2, b2), F4(0)))
    return dict(A1=A1, A2=A2, O3=t32(lin(A2, W3, b3)))


def mlp_bwd_emulate(dO3, A1, A2, P0, P1, order="seq", towers=(0, 1), mask=lambda a: a > 0):
    """One net -> dict(dA2, dA1 [2][n][128], dH [n][D]).  Mutants: dH from `towers` only; mask (the ReLU mask from the stored activation)."""
    dA2, dA1 = [], []
    for tw, P in enumerate((P0, P1)):
        dA2.append(torch.where(mask(A2[tw]), t32(dot32(dO3[tw], P[4].t(), order)), torch.zeros(())))
        dA1.append(torch.where(mask(A1[tw]), t32(dot32(dA2[tw], P[2].t(), order)), torch.zeros(())))
    Ps = (P0, P1)
    dH = t32(dot32(torch.cat([dA1[t] for t in towers], 1), torch.cat([Ps[t][0].t() for t in towers], 1), order))
    return dict(dA2=torch.stack(dA2), dA1=torch.stack(dA1), dH=dH)


def old_metric(got, ref):
    """max|got - ref| / max|ref|: the metric of the fused-kernel tests in tests/test_kernels_gpu.py (bar 1e-5 forward, 2e-5 elsewhere)."""
    return bp.old_metric(got, ref)
