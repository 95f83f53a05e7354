"""Element-wise float64 parity bound for the loss, policy-head and optimiser kernels — the bound, stated once ("loss / head /
optimiser parity").  The kernels: ppo_loss_body (cadre_kernels.hip: cadre_ppo_loss, _stats, _hp, _stats_hp, _ord), bc_loss_kernel
(imitation.hip), ppo_demo_loss_kernel (demo_mix.hip), the head's front (cadre_categorical_dist / _eval, cadre_sample and their _ord twins)
and clip + Adam (cadre_clip_adam, _graph, _norms + _apply).

No stored intermediate separates the stages of these kernels: a row goes from raw logits to its gradient in registers, through expf, logf
and divides, so the c_bar 2^-24 mag ruler of tests/f32_parity.py does not fit.  Instead every statement of a kernel's row body is evaluated in
float64 on (value, error) pairs (class VE, a sibling of update_parity.VM) that carry a RUNNING FIRST-ORDER ERROR BOUND:

    every operation          adds half an fp32 ulp of its own result, 2^-24 |v|, and propagates its operands' errors to first order
                             (a + b: ea + eb;  a b: |a| eb + |b| ea (+ ea eb);  a / b: ea / |b| + |a| eb / b^2)
    exp                      multiplies the incoming absolute error by the result and adds T_EXP ulps of the result plus the floor 2^-126
                             (where expf underflows the kernel holds 0 or a subnormal, float64 a number below the smallest normal fp32)
    log                      adds err / |x| plus T_LOG ulps of the result
    sqrt                     err / (2 sqrt x) plus half an ulp (correctly rounded, as the divide: the build passes no fast-math flag)
    a wave sum over 64 lanes adds six roundings of sum|terms| (the depth of the shuffle tree; a ladder scan has the same depth)

one ulp := 2^-23 |v|.  An operation whose operands carry no error and whose float64 result is an fp32 number is exact in fp32 too and adds
nothing (v - v_old = 0, 0 + clip, 0.25 * 0.25, a count): that is what keeps the planted ties below exact.  A quotient whose divisor is 2^127 or
more (1 / (1 + expf(x)) where expf overflows to +inf) gets |a| 2^-126 on top.  expf(0) = 1 and logf(1) = 0 are taken as exact (a head
with one bin then has lg = 0, p = 1, H = 0 and ratio = expf(-old_logp) without error, which plants a ratio on the clamp).  The test is

    |got - v64|  <=  err64        for EVERY stored element,

no FACTOR, no sampled subset, no exempt share; every checked output is finite; an element whose bound is zero must be bit-equal to v64, which
for everything the kernels write without arithmetic (the other commands' nets, rows with a bad command or label, columns K .. ldl-1, an
empty or gated Adam range) means an exact zero or the untouched value.  What the header does not say is written must keep the sentinel
the buffer was filled with.

T_EXP = update_parity.T_EXP = 3 and T_LOG = 3 ulps: the OpenCL full-profile limits of single-precision exp and log, which the device math
library (OCML) is built to.  As update_parity.py says of T_EXP: no accuracy table of the library's own is in the ROCm tree used for
development, the figures are the specification's as remembered and are NOT taken from the kernels' output.  The GPU tests print the worst
observed err / bound per case; an observed value is recorded, never used as the bar.

Each kernel's row body is written ONCE below (front, ord_logits, ord_backward, ppo_row, bc_row — also the demonstration row of the mixed kernel —, adam_row), generic over an
operand namespace X: X64 (float64 arrays: the reference), XVE (pairs: the bound) and X32 (fp32 numpy: the emulation that serves
tests/test_loss_parity_cpu.py, in two summation orders — "tree", the kernels' shuffle tree and ladder scans, and "seq", strictly
sequential).  The `mut` argument names one-statement mutants of the body.

Branch points (min(s1, s2), the clamp of the ratio, max(vl, vlc), the clamp of v - v_old, the > clip counts, the top-1 count, mode, the
sampled index) are not smooth.  XVE compares with a tolerance: a comparison of two pairs is UNSURE when their float64 values lie within
the sum of their error bounds (and that sum is not zero: two exact operands compare exactly).  Where a comparison is unsure, the result
is the float64 branch with the bound widened to the hull of the admissible branches (e = max(e_chosen, e_other + |v_other - v_chosen|));
torch's 0.5 / 0.5 split of a tie lies inside that hull.  A row is AMBIGUOUS when an unsure comparison selects between branches that
differ by more than their own bounds (its hull is then wide: an ambiguous row is not skipped, its outputs must be in the hull); a count
then has bound 1 for that row (it must lie between the counts with the row resolved either way) and an index must be one of the
candidates.  Most unsure comparisons are harmless: an unclipped row has s1 == s2 identically, and inside the value clamp
v_old + (v - v_old) differs from v by rounding only.  Condition: at most one ambiguous row per case that was not planted on a tie on
purpose, asserted from the float64 pairs alone (tests/test_loss_parity_cpu.py).

Sums (losses[], demo_losses[], the stats rows): the sum of the per-row bounds, plus n_add 2^-24 sum|term| with n_add counted from the code
(3 in-wave adds over 4 rows, 2 across waves, 2 nblk by the last arriver), plus the final coefficient products as pair operations.

Plain helper module (no GPU, no fixtures)."""
import math

import numpy as np

from tests import update_parity as up

F4, F8 = np.float32, np.float64
U = 2.0 ** -24
ULP = 2.0 ** -23
FLOOR = 2.0 ** -126
T_EXP = up.T_EXP
T_LOG = 3.0
ORD_EPS = F4(1e-8)          # CADRE_ORD_EPS
SENT = F4(-7.5)             # sentinel the output buffers are filled with


# ----------------------------------------------------------------------------- (value, error) pairs
def _rnd(v, *errs):
    """Half an fp32 ulp of the result — nothing where the operation is exact in fp32 (exact operands, fp32-representable result)."""
    exact = np.ones(np.shape(v), bool)
    for e in errs:
        exact = exact & (e == 0)
    with np.errstate(over="ignore", invalid="ignore"):
        rep = np.asarray(v, F8).astype(F4).astype(F8) == v
    return np.where(exact & rep, 0.0, U * np.abs(v))


class VE:
    """A float64 value with a running first-order bound on the error of its fp32 evaluation."""
    __array_priority__ = 100

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=F8)
        self.e = np.zeros(self.v.shape) if e is None else np.zeros(self.v.shape) + np.asarray(e, dtype=F8)

    @staticmethod
    def of(x):
        return x if isinstance(x, VE) else VE(x)

    @property
    def shape(self):
        return self.v.shape

    def __getitem__(self, i):
        return VE(self.v[i], self.e[i])

    def __neg__(self):
        return VE(-self.v, self.e)

    def __add__(self, o):
        o = VE.of(o)
        v = self.v + o.v
        return VE(v, self.e + o.e + _rnd(v, self.e, o.e))

    def __sub__(self, o):
        o = VE.of(o)
        v = self.v - o.v
        return VE(v, self.e + o.e + _rnd(v, self.e, o.e))

    def __rsub__(self, o):
        return VE.of(o) - self

    def __mul__(self, o):
        o = VE.of(o)
        v = self.v * o.v
        return VE(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + _rnd(v, self.e, o.e))

    def __truediv__(self, o):
        o = VE.of(o)
        with np.errstate(over="ignore"):
            v = self.v / o.v
            e = self.e / np.abs(o.v) + np.abs(v) * (o.e / np.abs(o.v)) + _rnd(v, self.e, o.e)
        return VE(v, e + np.where(np.abs(o.v) >= 2.0 ** 127, np.abs(self.v) * FLOOR, 0.0))

    def __rtruediv__(self, o):
        return VE.of(o) / self

    __radd__, __rmul__ = __add__, __mul__


def _int_sum(a, axis):
    """A sum of error-free integers below 2^24 (a count): exact in fp32 in any order."""
    return (a.e == 0).all(axis) & (a.v == np.round(a.v)).all(axis) & (np.abs(a.v).sum(axis) < 2 ** 24)


class FZ:
    """A comparison of pairs: its float64 outcome and whether the error bounds leave it open."""

    def __init__(self, val, unsure):
        self.val, self.unsure = val, unsure


# ----------------------------------------------------------------------------- operand namespaces
class X64:
    """float64 arrays: the reference.  Lanes are the last axis; a sum / max / scan runs over it."""
    dtype = F8

    def __init__(self, order="tree"):
        self.order = order

    def c(self, x):
        return np.asarray(x, dtype=self.dtype)

    def exp(self, a):
        with np.errstate(over="ignore", under="ignore"):
            return np.exp(a)

    def log(self, a):
        return np.log(a)

    def sqrt(self, a):
        return np.sqrt(a)

    def absv(self, a):
        return np.abs(a)

    def sum(self, a):
        return a.sum(-1)

    def max(self, a):
        return a.max(-1)

    def scan_up(self, a):
        return np.cumsum(a, -1)

    def scan_down(self, a):
        return np.cumsum(a[..., ::-1], -1)[..., ::-1]

    def shift_left(self, a):                      # lane j takes lane j + 1, the last lane 0
        return np.concatenate([a[..., 1:], np.zeros_like(a[..., :1])], -1)

    def shift_right(self, a):
        return np.concatenate([np.zeros_like(a[..., :1]), a[..., :-1]], -1)

    def take(self, a, idx):
        return np.take_along_axis(a, np.broadcast_to(idx, a.shape[:-1] + idx.shape[-1:]), -1)

    def where(self, c, a, b):                     # c: a plain bool array (structure: lane == a, a zero target)
        return np.where(c, a, b)

    def lt(self, a, b):
        return a < b

    def gt(self, a, b):
        return a > b

    def le(self, a, b):
        return a <= b

    def ge(self, a, b):
        return a >= b

    def land(self, p, q):
        return p & q

    def fwhere(self, fz, a, b):
        return np.where(fz, a, b)

    def fmin(self, a, b):
        return np.minimum(a, b)

    def fmax(self, a, b):
        return np.maximum(a, b)

    def count(self, fz):
        return np.where(fz, self.dtype(1), self.dtype(0))


class X32(X64):
    """fp32 numpy: every operation rounded to fp32; expf / logf as np.float32 of the float64 function.  order "tree": wave sums as the
    xor-shuffle tree over 64 lanes (32, 16, .. 1), scans as the shuffle ladders of ordinal.h; "seq": strictly sequential."""
    dtype = F4

    def exp(self, a):
        assert a.dtype == F4
        with np.errstate(over="ignore", under="ignore"):
            return np.exp(a.astype(F8)).astype(F4)

    def log(self, a):
        assert a.dtype == F4
        with np.errstate(divide="ignore"):
            return np.log(a.astype(F8)).astype(F4)

    def sqrt(self, a):
        assert a.dtype == F4
        return np.sqrt(a)

    def sum(self, a):
        assert a.dtype == F4
        if self.order == "seq":
            return np.cumsum(a, -1, dtype=F4)[..., -1]
        v = np.concatenate([a, np.zeros(a.shape[:-1] + (64 - a.shape[-1],), F4)], -1)
        o = 32
        while o:
            v = v[..., :o] + v[..., o:]
            o >>= 1
        return v[..., 0]

    def scan_up(self, a):
        assert a.dtype == F4
        if self.order == "seq":
            return np.cumsum(a, -1, dtype=F4)
        v, o = a.copy(), 1
        while o < a.shape[-1]:
            v = np.concatenate([v[..., :o], v[..., o:] + v[..., :-o]], -1)
            o <<= 1
        return v

    def scan_down(self, a):
        return self.scan_up(a[..., ::-1])[..., ::-1]


class XVE(X64):
    """Pairs: the float64 reference with its bound.  amb [rows]: the ambiguous rows met so far (first axis = rows)."""

    def __init__(self, n_rows, order="tree"):
        self.order = order
        self.amb = np.zeros(n_rows, bool)

    def c(self, x):
        return VE(x)

    def exp(self, a):
        with np.errstate(over="ignore", under="ignore"):
            v = np.exp(np.minimum(a.v, 700.0))
            return VE(v, np.where((a.v == 0) & (a.e == 0), 0.0, v * np.expm1(np.minimum(a.e, 50.0)) + T_EXP * ULP * v + FLOOR))

    def log(self, a):
        v = np.log(a.v)
        return VE(v, np.where((a.v == 1) & (a.e == 0), 0.0, a.e / np.abs(a.v) + T_LOG * ULP * np.abs(v)))

    def sqrt(self, a):
        v = np.sqrt(a.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            return VE(v, np.where(a.e > 0, a.e / (2 * v), 0.0) + _rnd(v, a.e))

    def absv(self, a):
        return VE(np.abs(a.v), a.e)

    def sum(self, a):
        v = a.v.sum(-1)
        return VE(v, a.e.sum(-1) + np.where(_int_sum(a, -1), 0.0, 6 * U * np.abs(a.v).sum(-1)))

    def max(self, a):
        return VE(a.v.max(-1), a.e.max(-1))

    def scan_up(self, a):
        return VE(np.cumsum(a.v, -1), np.cumsum(a.e, -1) + 6 * U * np.cumsum(np.abs(a.v), -1))

    def scan_down(self, a):
        r = self.scan_up(a[..., ::-1])
        return r[..., ::-1]

    def shift_left(self, a):
        return VE(X64.shift_left(self, a.v), X64.shift_left(self, a.e))

    def shift_right(self, a):
        return VE(X64.shift_right(self, a.v), X64.shift_right(self, a.e))

    def take(self, a, idx):
        return VE(X64.take(self, a.v, idx), X64.take(self, a.e, idx))

    def where(self, c, a, b):
        a, b = VE.of(a), VE.of(b)
        return VE(np.where(c, a.v, b.v), np.where(c, a.e, b.e))

    def _cmp(self, a, b, op):
        a, b = VE.of(a), VE.of(b)
        tol = a.e + b.e
        return FZ(op(a.v, b.v), (np.abs(a.v - b.v) <= tol) & (tol > 0))

    def lt(self, a, b):
        return self._cmp(a, b, np.less)

    def gt(self, a, b):
        return self._cmp(a, b, np.greater)

    def le(self, a, b):
        return self._cmp(a, b, np.less_equal)

    def ge(self, a, b):
        return self._cmp(a, b, np.greater_equal)

    def land(self, p, q):
        return FZ(p.val & q.val, (p.unsure & (q.val | q.unsure)) | (q.unsure & (p.val | p.unsure)))

    def _mark(self, rows):
        rows = np.asarray(rows)
        while rows.ndim > 1:
            rows = rows.any(-1)
        self.amb = self.amb | np.broadcast_to(rows, self.amb.shape)

    def fwhere(self, fz, a, b):
        a, b = VE.of(a), VE.of(b)
        cv, ce = np.where(fz.val, a.v, b.v), np.where(fz.val, a.e, b.e)
        ov, oe = np.where(fz.val, b.v, a.v), np.where(fz.val, b.e, a.e)
        gap = np.abs(ov - cv)
        uns = np.broadcast_to(fz.unsure, cv.shape)
        self._mark(uns & (gap > ce + oe))
        return VE(cv, np.where(uns, np.maximum(ce, oe + gap), ce))

    def fmin(self, a, b):
        return self.fwhere(self.lt(a, b), a, b)

    def fmax(self, a, b):
        return self.fwhere(self.gt(a, b), a, b)

    def count(self, fz):
        self._mark(fz.unsure)
        return VE(np.where(fz.val, 1.0, 0.0), np.where(fz.unsure, 1.0, 0.0))


def split(a):
    """pair or array -> (float64 value, bound or None)."""
    return (a.v, a.e) if isinstance(a, VE) else (np.asarray(a), None)


# ----------------------------------------------------------------------------- the row bodies, each written once
def ord_logits(X, x, rk, mut=()):
    """ordinal.h ord_logits on lanes 0 .. K-1 -> (bin logits, s, t)."""
    one, eps = X.c(1.0), X.c(ORD_EPS)
    s = one / (one + X.exp(-x))
    t = (one - s) if "one_minus_s" in mut else one / (one + X.exp(x))
    if "ord_no_eps" in mut:
        u, w = X.log(s), X.log(t)
    elif "ord_eps_outside" in mut:
        u, w = X.log(s) + eps, X.log(t) + eps
    else:
        u, w = X.log(s + eps), X.log(t + eps)
    z = X.scan_up(u) + X.scan_down(X.shift_left(w))
    return X.take(z, rk), s, t


def ord_backward(X, g, s, t, rk, mut=()):
    """ordinal.h ord_backward: g = d total / d bin logit -> d total / d threshold unit."""
    eps = X.c(ORD_EPS)
    binv = np.argsort(rk)
    G = X.take(g, binv)
    pre = X.shift_right(X.scan_up(G))
    suf = X.scan_down(G)
    st = s * t
    if "ord_no_eps" in mut:
        a, b = st / s, st / t
    else:
        a, b = st / (s + eps), st / (t + eps)
    return a * suf - b * pre


def front(X, x, rk=None, mut=()):
    """The shared front of every kernel here: raw [n][K] -> normalised logits lg, probabilities pk [n][K], entropy H [n] (and the two
    sigmoids of an ordinal head)."""
    s = t = None
    if rk is not None:
        x, s, t = ord_logits(X, x, rk, mut)
    mx = X.max(x)
    se = X.sum(X.exp(x - mx[..., None]))
    lse = mx + X.log(se)
    lg = x - lse[..., None]
    mx2 = X.max(lg)
    e2 = X.exp(lg - mx2[..., None])
    se2 = X.sum(e2)
    pk = e2 / se2[..., None]
    H = -X.sum(pk * lg)
    return lg, pk, H, s, t


def _onehot(a, K):
    return np.arange(K)[None, :] == np.asarray(a)[:, None]


def ppo_row(X, x, a, v, ov, R, olp, A, hp, rk=None, mut=()):
    """ppo_loss_body from the raw logits of the rows' own net to the gradients and the per-row terms of the sums.  x [n][K], the rest [n]
    (typed by X.c), a int [n]; hp = (clip, value_coeff, clip_coeff, ent_coeff, inv_b) as fp32 numbers."""
    clip, vc, cc, ec, inv_b = (X.c(F4(h)) for h in hp)
    one, half, zero, two = X.c(1.0), X.c(0.5), X.c(0.0), X.c(2.0)
    K = x.shape[-1]
    lg, pk, H, s, t = front(X, x, rk, mut)
    lp = X.take(lg, np.asarray(a)[:, None])[..., 0]
    lr = lp - olp
    ratio = X.exp(lr)
    s1 = ratio * A
    lo, hi = one - clip, one + clip
    rc = X.fmin(X.fmax(ratio, lo), hi)
    s2 = rc * A
    dv = v - ov
    dvc = X.fmin(X.fmax(dv, -clip), clip)
    vpc = ov + dvc
    d1, d2 = v - R, vpc - R
    vl, vlc = d1 * d1, d2 * d2
    terms = dict(act=-X.fmin(s1, s2), val=X.fmax(vl, vlc), ent=H,
                 kl=(ratio - one) - lr, okl=-lr, cf=X.count(X.gt(X.absv(ratio - one), clip)), vcf=X.count(X.gt(X.absv(dv), clip)),
                 r=ratio, alr=X.absv(lr))
    if "in_ratio_excl" in mut:
        in_ratio = X.land(X.gt(ratio, lo), X.lt(ratio, hi))
    else:
        in_ratio = X.land(X.ge(ratio, lo), X.le(ratio, hi))
    tie = half * A + X.fwhere(in_ratio, half * A, zero)
    dmin = X.fwhere(X.lt(s1, s2), A, X.fwhere(X.gt(s1, s2), X.fwhere(in_ratio, A, zero), tie))
    dlp = cc * inv_b * (-dmin) * ratio
    if "in_v_excl" in mut:
        in_v = X.land(X.gt(dv, -clip), X.lt(dv, clip))
    else:
        in_v = X.land(X.ge(dv, -clip), X.le(dv, clip))
    g1, g2 = two * d1, X.fwhere(in_v, two * d2, zero)
    vtie = g1 if "tie_one_side" in mut else half * g1 + half * g2
    dmax = X.fwhere(X.gt(vl, vlc), g1, X.fwhere(X.lt(vl, vlc), g2, vtie))
    dval = vc * inv_b * half * dmax
    dH = -ec * inv_b
    hit = X.where(_onehot(a, K), one, zero)
    if "ent_no_H" in mut:
        et = -pk * lg
    else:
        et = -pk * (lg + H[..., None])
    if "ent_skip_small" in mut:
        et = X.where(split(pk)[0] < 1e-6, zero, et)
    gk = dlp[..., None] * (hit - pk) + dH * et
    if rk is not None:
        gk = ord_backward(X, gk, s, t, rk, mut)
    return gk, dval, terms


def _target(X, a, K, eps, mut=()):
    one = X.c(1.0)
    t_off = eps / X.c(F4(K - 1 if "t_off_km1" in mut else K))
    t_on = (one - eps) + t_off
    return X.where(_onehot(a, K), t_on, t_off)


def _top1(X, pk, a):
    """The top-1 hit of bc_loss_kernel: the lowest index among the largest probabilities equals the action."""
    v, e = split(pk)
    top = np.argmax(v, -1)
    hit = top == np.asarray(a)
    if e is None:
        return X.count(hit)
    n = np.arange(v.shape[0])
    rival = (v[n, top][:, None] - v) <= (e[n, top][:, None] + e)   # bins the error bounds cannot tell from the largest
    rival[n, top] = False
    unsure = rival.any(-1) & (hit | rival[n, np.asarray(a)])
    return X.count(FZ(hit, unsure))


def bc_row(X, x, a, v, R, w, hp, rk=None, mut=(), demo=False):
    """bc_loss_kernel (demo = False; hp = (label_smoothing, bc_coeff, value_coeff, ent_coeff, inv_b)) and the demonstration row of
    ppo_demo_loss_kernel (demo = True: no entropy term; hp = (label_smoothing, demo_coeff, demo_value_coeff, 0, inv_bd))."""
    eps, bc, vc, ec, inv_b = (X.c(F4(h)) for h in hp)
    K = x.shape[-1]
    lg, pk, H, s, t = front(X, x, rk, mut)
    lp = X.take(lg, np.asarray(a)[:, None])[..., 0]
    tk = _target(X, a, K, eps, mut)
    live = _onehot(a, K) | (F4(hp[0]) != 0)                         # tk != 0
    ce = -X.sum(X.where(live, tk * lg, X.c(0.0)))
    dv = v - R
    terms = dict(val=w * (dv * dv), ce=w * ce, ent=w * H, top=_top1(X, pk, a), nll=-lp, H=H, adv=X.absv(dv), w=w, n=X.c(1.0) + X.c(0.0) * w)
    wb = w * (X.c(F4(hp[4])) if "demo_inv_b" not in mut else X.c(F4(mut["demo_inv_b"])))
    dval = (vc * inv_b * dv) if "w_missing_dvalues" in mut else vc * wb * dv
    if demo:
        gk = wb[..., None] * (bc * (pk - tk))
    else:
        if "ent_no_H" in mut:
            et = pk * lg
        else:
            et = pk * (lg + H[..., None])
        if "ent_skip_small" in mut:
            et = X.where(split(pk)[0] < 1e-6, X.c(0.0), et)
        gk = wb[..., None] * (bc * (pk - tk) + ec * et)
    if rk is not None:
        gk = ord_backward(X, gk, s, t, rk, mut)
    return gk, dval, terms


def adam_row(X, p, g, m, v, total, hp, mut=()):
    """adam_kernel / adam_dev_kernel_body on the elements of one segment.  total: sqrt of the segment's square norm (float64 number);
    hp = (max_norm, step_size, w1, beta2, w2, bc2_sqrt, eps) as fp32 numbers.  -> (p', m', v')."""
    maxn, step, w1, beta2, w2, bc2s, eps = (h if isinstance(h, VE) else X.c(F4(h)) for h in hp)
    if isinstance(X, XVE):
        tot = VE(total, U * abs(total))                             # (float)sqrt(norms2[mdl])
    else:
        tot = X.c(F4(total)) if X.dtype is F4 else X.c(total)
    coef = X.fmin(maxn / (tot + X.c(F4(1e-6))), X.c(1.0))
    gi = g * coef
    m1 = m + w1 * (gi - m)
    gv = g if "clip_m_only" in mut else gi
    if "w2_beta2_swapped" in mut:
        v1 = v * w2 + beta2 * (gv * gv)
    else:
        v1 = v * beta2 + w2 * (gv * gv)
    if "eps_inside" in mut:
        den = (X.sqrt(v1) + eps) / bc2s
    else:
        den = X.sqrt(v1) / bc2s + eps
    return p - step * (m1 / den), m1, v1


# ----------------------------------------------------------------------------- the sums of the loss kernels
def n_add(nblk):
    """Additions between a row's term and the stored sum: 3 in the wave (4 rows), 2 across the 4 waves, 2 nblk by the last arriver."""
    return 3 + 2 + 2 * nblk


def reduce_rows(X, term, B, per_head, use_max=False):
    """term: typed [2][B] (zeros where a row adds nothing) -> the kernel's sum over both heads ([] typed) or per head ([2]).  X32 "tree":
    the kernel's own order — sequentially over the 4 rows of a wave, (w0 + w1) + (w2 + w3), then the workgroups in index order."""
    nblk = (B + 15) // 16
    if isinstance(X, XVE):
        ax = -1 if per_head else None
        v, e = term.v, term.e
        if use_max:
            i = np.argmax(v, -1)
            return VE(np.take_along_axis(v, i[:, None], -1)[:, 0], e.max(-1))
        s = v.sum(ax)
        return VE(s, e.sum(ax) + np.where(_int_sum(term, ax), 0.0, n_add(nblk) * U * np.abs(v).sum(ax)))
    t = np.asarray(term)
    if use_max:
        return t.max(-1)
    if type(X) is X64:
        return t.sum(-1) if per_head else t.sum()
    if X.order == "seq":
        return np.cumsum(t, -1, dtype=F4)[:, -1] if per_head else np.cumsum(t.reshape(-1), dtype=F4)[-1]
    pad = np.zeros((2, nblk * 16), F4)
    pad[:, :B] = t
    w = np.cumsum(pad.reshape(2, nblk, 4, 4), -1, dtype=F4)[..., -1]
    blk = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])                   # [2][nblk]
    return np.cumsum(blk, -1, dtype=F4)[:, -1] if per_head else np.cumsum(blk.reshape(-1), dtype=F4)[-1]


# ----------------------------------------------------------------------------- test data
def rank_table(K, ordinal):
    """[64] int32 rank table of one head: -1 first for a categorical head; for an ordinal head the shipped steer table's shape for K = 33
    (through ppo_agent's ordinal_rank: non-monotone), otherwise the same interleaving cut to K bins."""
    out = np.full(64, -1, np.int32)
    if not ordinal:
        return out
    n = (K + 1) // 2
    ctl = {i: float(i - n // 2) for i in range(n)}                           # ascending block, then +, -, +, - outwards
    for j, k in enumerate(range(n, K)):
        ctl[k] = (n + j // 2) * (1.0 if j % 2 == 0 else -1.0) + (0.5 if j % 2 else 0.0)
    if K == 33:
        from tests.test_ordinal_cpu import shipped_steer
        ctl = shipped_steer()
    from cadre_amd.ppo_agent.models import ordinal_rank
    out[:K] = ordinal_rank(ctl)
    return out


FAMILIES = ("plain", "plain", "plain", "spike", "equal", "shift", "plain", "unit20")


def raw_rows(r, n, K, scale, ordinal):
    """fp32 [n][K] raw tower outputs, the families by row index: N(0, scale); one logit 60 above the rest; all equal; shifted by +1000 (an
    ordinal head saturates every unit there: expf overflows); ordinal heads also a row with a quarter of its units at +-20."""
    x = (r.standard_normal((n, K)) * scale).astype(F4)
    for i in range(n):
        fam = FAMILIES[i % len(FAMILIES)]
        if fam == "spike":
            x[i, r.randint(K)] += F4(60.0)
        elif fam == "equal":
            x[i, :] = x[i, 0]
        elif fam == "shift":
            x[i, :] += F4(1000.0)
        elif fam == "unit20" and ordinal:
            j = r.randint(K, size=max(1, K // 4))
            x[i, j] = np.where(r.random_sample(j.shape) < 0.5, F4(20.0), F4(-20.0))
    return x


class LossCase:
    """Operands of one loss-kernel case, as the kernels address them.  kind: "ppo", "bc" or "mix"."""

    def __init__(self, seed, kind, B, Ks, C, ldl, scale=1.0, ordinal=(False, False), clip=0.1, ent_coeff=0.01, smoothing=0.1,
                 weights=True, demo_share=0.4, empty=None):
        r = np.random.RandomState(seed)
        self.kind, self.B, self.Ks, self.C, self.ldl, self.seed = kind, B, tuple(Ks), C, ldl, seed
        self.ldv, self.l_ns, self.v_ns = 3, B * ldl + 24, B * 3 + 5                 # no two strides coincide
        self.guard = 40
        self.ord = np.stack([rank_table(Ks[0], ordinal[0]), rank_table(Ks[1], ordinal[1])])
        self.ordinal = tuple(ordinal)
        self.hp = dict(clip=F4(clip), value_coeff=F4(0.5), clip_coeff=F4(1.0), ent_coeff=F4(ent_coeff), inv_b=F4(1.0 / max(1, B)),
                       smoothing=F4(smoothing), bc_coeff=F4(0.8), demo_coeff=F4(0.3), demo_value_coeff=F4(0.2), inv_bd=F4(1.0 / max(1, B // 3 + 1)))
        self.logits = np.full(2 * C * self.l_ns + self.guard, SENT, F4)
        self.values = np.full(2 * C * self.v_ns + self.guard, SENT, F4)
        for net in range(2 * C):
            K = Ks[net // C]
            blk = np.zeros((B, ldl), F4)
            blk[:, :K] = raw_rows(r, B, K, scale, ordinal[net // C])
            blk[:, K:] = F4(3.25)                                                   # pitch columns: never read
            self.logits[net * self.l_ns: net * self.l_ns + B * ldl] = blk.reshape(-1)
            self.values[net * self.v_ns: net * self.v_ns + B * self.ldv: self.ldv] = r.standard_normal(B).astype(F4)
        self.actions = np.stack([r.randint(0, K, B) for K in Ks]).astype(np.int64)
        self.cmds = r.randint(0, C, (2, B)).astype(np.int32)
        self.kindrow = np.zeros((2, B), np.int32)
        if kind == "bc":
            self.kindrow[:] = 1
        elif kind == "mix":
            # a sorted layout: pos [2][B] a permutation per head; unsorted rows B_ppo .. B-1 are the demonstration rows
            self.B_ppo = B - int(round(B * demo_share))
            self.pos = np.stack([r.permutation(B) for _ in range(2)]).astype(np.int32)
            for h in range(2):
                self.kindrow[h, self.pos[h, self.B_ppo:]] = 1
            if empty == "no_ppo_head0":
                self.kindrow[0, :] = 1
            if empty == "no_demo_head1":
                self.kindrow[1, :] = 0
        # out-of-range rows: commands -1 and C; on the demonstration paths actions -1 and K
        if B >= 15:
            self.cmds[0, 2], self.cmds[1, 5] = -1, C
            self.cmds[1, B - 1] = -1
            for h in range(2):
                d = np.flatnonzero(self.kindrow[h] == 1)
                if d.size >= 2:
                    self.actions[h, d[0]], self.actions[h, d[-1]] = -1, Ks[h]
        self.old_v = r.standard_normal((2, B)).astype(F4)
        self.rets = r.standard_normal((2, B)).astype(F4)
        self.adv = r.standard_normal((2, B)).astype(F4)
        self.weights = (r.uniform(0.25, 3.0, (2, B)).astype(F4)) if weights else None
        if kind == "mix":
            wt = r.uniform(0.25, 3.0, (2, B)).astype(F4)
            self.adv = np.where(self.kindrow == 1, wt, self.adv)
        # planted rows with exactly representable ties (PPO rows only): v == v_old; v_old = 0, v = (float)clip; adv == 0; and, where clip
        # is a power of two, v_old = 0, v = 5 clip, R = 3 clip: (v - R)^2 == (v_old + clip - R)^2 outside the clamp
        self.planted = np.zeros((2, B), bool)
        if B >= 15:
            spots = [(0, 1, "veq"), (1, 3, "vclip"), (0, 4, "adv0"), (1, 7, "vtie")]
            for h, b, what in spots:
                if self.kindrow[h, b] != 0 or not self.row_ok(h, b):
                    continue
                i = (h * C + self.cmds[h, b]) * self.v_ns + b * self.ldv
                if what == "veq":
                    self.old_v[h, b] = self.values[i]
                elif what == "vclip":
                    self.old_v[h, b], self.values[i] = 0, F4(clip)
                elif what == "adv0":
                    self.adv[h, b] = 0
                elif what == "vtie" and math.frexp(clip)[0] == 0.5:
                    self.old_v[h, b], self.values[i], self.rets[h, b] = 0, F4(5 * clip), F4(3 * clip)
                else:
                    continue
                self.planted[h, b] = True
        for h in range(2):                                                          # rows whose logits are all equal tie the top-1 and the mode
            for b in range(B):
                if FAMILIES[b % len(FAMILIES)] == "equal" and Ks[h] > 1:
                    self.planted[h, b] = True
        # old_logp: the float64 log-prob plus N(0, 0.3): both clip sides and the unclipped branch occur
        self.old_lp = np.zeros((2, B), F4)
        X = X64()
        for h in range(2):
            rows = self.rows(h, None)
            if rows.size:
                a = np.clip(self.actions[h, rows], 0, Ks[h] - 1)
                lg = front(X, self.own_logits(h, rows).astype(F8), self.rk(h))[0]
                self.old_lp[h, rows] = (lg[np.arange(rows.size), a] + 0.3 * r.standard_normal(rows.size)).astype(F4)

        if clip == 0 and Ks[0] == 1 and B >= 15 and kind == "ppo" and self.row_ok(0, 6):
            self.old_lp[0, 6] = 0                                                   # K = 1: lp = 0, ratio = expf(0) = 1 = 1 - clip = 1 + clip
            self.planted[0, 6] = True

    @classmethod
    def from_arrays(cls, kind, logits, values, actions, cmds, rets, Ks, C, ranks, hp, old_v=None, old_lp=None, adv=None, kindrow=None,
                    weights=None):
        """The inputs of an existing test (logits [2C][B][64], values [2C][B], sample arrays [2][B]; ranks: lists or None per head)."""
        self = object.__new__(cls)
        B = int(np.shape(actions)[1])
        self.kind, self.B, self.Ks, self.C, self.ldl, self.seed = kind, B, tuple(Ks), C, 64, -1
        self.ldv, self.l_ns, self.v_ns, self.guard = 1, B * 64, B, 0
        self.ordinal = tuple(r is not None for r in ranks)
        self.ord = np.full((2, 64), -1, np.int32)
        for h, r in enumerate(ranks):
            if r is not None:
                self.ord[h, :Ks[h]] = r
        self.hp = {k: F4(v) for k, v in hp.items()}
        f = lambda t, dt=F4: None if t is None else np.ascontiguousarray(np.asarray(t), dtype=dt)
        self.logits, self.values = f(logits).reshape(-1), f(values).reshape(-1)
        self.actions, self.cmds, self.rets = f(actions, np.int64), f(cmds, np.int32), f(rets)
        z = np.zeros((2, B), F4)
        self.old_v, self.old_lp, self.adv = (z if t is None else f(t) for t in (old_v, old_lp, adv))
        self.kindrow = np.full((2, B), 1 if kind == "bc" else 0, np.int32) if kindrow is None else f(kindrow, np.int32)
        self.weights, self.planted = f(weights), np.zeros((2, B), bool)
        return self

    def row_ok(self, h, b):
        return 0 <= self.cmds[h, b] < self.C

    def rk(self, h):
        return self.ord[h, :self.Ks[h]].astype(np.int64) if self.ordinal[h] else None

    def rows(self, h, demo):
        """Rows of head h that count: demo None — any kind (command in range); False — PPO rows; True — demonstration rows with a label."""
        ok = (self.cmds[h] >= 0) & (self.cmds[h] < self.C)
        if demo is None:
            return np.flatnonzero(ok)
        if demo:
            return np.flatnonzero(ok & (self.kindrow[h] == 1) & (self.actions[h] >= 0) & (self.actions[h] < self.Ks[h]))
        return np.flatnonzero(ok & (self.kindrow[h] == 0))

    def own_logits(self, h, rows):
        net = h * self.C + self.cmds[h, rows]
        idx = (net * self.l_ns + rows * self.ldl)[:, None] + np.arange(self.Ks[h])[None, :]
        return self.logits[idx]

    def own_values(self, h, rows):
        return self.values[(h * self.C + self.cmds[h, rows]) * self.v_ns + rows * self.ldv]

    def tag(self):
        return "%s B %d K %s C %d ldl %d ord %s seed %d" % (self.kind, self.B, self.Ks, self.C, self.ldl, "".join("o" if o else "c" for o in self.ordinal), self.seed)


def run_loss(case, X, hp=None, stats=True, grad=True, weights=True, mut=()):
    """One launch of the case's kernel in the arithmetic of X -> dict of typed outputs: dlogits / dvalues (flat buffers: SENT where the
    emulation wrote nothing; pairs hold (0, 0) there), losses [3], stats [2][6], demo_losses [2], demo_stats [2][6]; with XVE also
    `amb` [2][B].  hp overrides case.hp (the `_hp` forms).  mut: a set of mutant names, or a dict for the ones that carry a value."""
    hpv = dict(case.hp)
    hpv.update(hp or {})
    B, C, ldl = case.B, case.C, case.ldl
    pair = X is XVE
    mk = (lambda n: XVE(n)) if pair else (lambda n: X)
    emul = isinstance(X, X32)
    out = {}
    if pair:
        dl, dv = VE(np.zeros(case.logits.size)), VE(np.zeros(case.values.size))
    else:
        dt = X.dtype
        dl, dv = np.full(case.logits.size, SENT, dt), np.full(case.values.size, SENT, dt)
        if grad:
            for net in range(2 * C):
                for b in range(B):
                    dl[net * case.l_ns + b * ldl: net * case.l_ns + (b + 1) * ldl] = 0
                    dv[net * case.v_ns + b * case.ldv] = 0
    amb = np.zeros((2, B), bool)
    names_p = ("val", "act", "ent", "kl", "okl", "cf", "vcf", "r", "alr")
    names_d = ("val", "ce", "ent", "top", "nll", "H", "adv", "w", "n")
    zero_t = (lambda: VE(np.zeros((2, B)))) if pair else (lambda: np.zeros((2, B), X.dtype))
    tp, td = {k: zero_t() for k in names_p}, {k: zero_t() for k in names_d}

    def put(buf, idx, val):
        v, e = split(val)
        if pair:
            buf.v[idx], buf.e[idx] = v, e
        else:
            buf[idx] = v

    for h in range(2):
        K = case.Ks[h]
        for demo in (False, True):
            if (demo and case.kind == "ppo") or (not demo and case.kind == "bc"):
                continue
            rows = case.rows(h, demo)
            if rows.size == 0:
                continue
            x_ = mk(rows.size)
            cst = x_.c if pair else (lambda a: np.asarray(a, x_.dtype))
            x = cst(case.own_logits(h, rows))
            v = cst(case.own_values(h, rows))
            a = case.actions[h, rows]
            if not demo:
                hp5 = (hpv["clip"], hpv["value_coeff"], hpv["clip_coeff"], hpv["ent_coeff"], hpv["inv_b"])
                gk, dval, terms = ppo_row(x_, x, a, v, cst(case.old_v[h, rows]), cst(case.rets[h, rows]), cst(case.old_lp[h, rows]),
                                          cst(case.adv[h, rows]), hp5, case.rk(h), mut)
                tdst = tp
            else:
                if case.kind == "bc":
                    w = cst(case.weights[h, rows]) if (weights and case.weights is not None) else cst(np.ones(rows.size, F4))
                    hp5 = (hpv["smoothing"], hpv["bc_coeff"], hpv["value_coeff"], hpv["ent_coeff"], hpv["inv_b"])
                else:
                    w = cst(case.adv[h, rows])
                    hp5 = (hpv["smoothing"], hpv["demo_coeff"], hpv["demo_value_coeff"], 0.0, hpv["inv_bd"])
                gk, dval, terms = bc_row(x_, x, a, v, cst(case.rets[h, rows]), w, hp5, case.rk(h), mut, demo=case.kind == "mix")
                tdst = td
            for k, t in terms.items():
                put(tdst[k], (h, rows), t)
            if pair:
                amb[h, rows] |= x_.amb
            if grad:
                net = h * C + case.cmds[h, rows]
                base = net * case.l_ns + rows * ldl
                if emul and "cols_unwritten" in mut:
                    for i in base:
                        dl[i + K: i + ldl] = SENT
                put(dl, base[:, None] + np.arange(K)[None, :], gk)
                put(dv, net * case.v_ns + rows * case.ldv, dval)
    out["dlogits"], out["dvalues"], out["amb"] = dl, dv, amb
    x_ = mk(2)
    c = x_.c if pair else (lambda a: np.asarray(a, x_.dtype))
    red = lambda t, per_head=False, use_max=False: reduce_rows(x_, t, B, per_head, use_max)
    half = c(0.5)
    if case.kind in ("ppo", "mix"):
        ib = c(hpv["inv_b"])
        out["losses"] = [c(hpv["value_coeff"]) * half * red(tp["val"]) * ib, c(hpv["clip_coeff"]) * red(tp["act"]) * ib,
                         c(hpv["ent_coeff"]) * red(tp["ent"]) * ib]
        if stats:
            st = [red(tp[k], True) * ib for k in ("kl", "okl", "cf", "vcf", "r")] + [red(tp["alr"], True, True)]
            out["stats"] = st                                                       # [6] of typed [2]
    if case.kind == "bc":
        ib = c(hpv["inv_b"])
        out["losses"] = [c(hpv["value_coeff"]) * half * red(td["val"]) * ib, c(hpv["bc_coeff"]) * red(td["ce"]) * ib,
                         c(hpv["ent_coeff"]) * red(td["ent"]) * ib]
        if stats:
            out["demo_stats"] = [red(td[k], True) * ib for k in ("top", "nll", "H", "adv", "w", "n")]
    if case.kind == "mix":
        ibd = c(hpv["inv_bd"])
        out["demo_losses"] = [c(hpv["demo_coeff"]) * red(td["ce"]) * ibd, c(hpv["demo_value_coeff"]) * half * red(td["val"]) * ibd]
        if stats:
            out["demo_stats"] = [red(td[k], True) * ibd for k in ("top", "nll", "H", "adv", "w", "n")]
    return out


def written(case):
    """(dlogits mask, dvalues mask) of what the headers say a GRAD launch writes: ldl columns of every row of every net, one value per row."""
    ml, mv = np.zeros(case.logits.size, bool), np.zeros(case.values.size, bool)
    for net in range(2 * case.C):
        ml[net * case.l_ns: net * case.l_ns + case.B * case.ldl] = True
        mv[net * case.v_ns: net * case.v_ns + case.B * case.ldv: case.ldv] = True
    return ml, mv


# ----------------------------------------------------------------------------- the check
class Report:
    """Collects |got - v64| <= err64 checks of one case; line() is the case's printed line."""

    def __init__(self, what):
        self.what, self.worst, self.where, self.n, self.bad = what, 0.0, "", 0, []

    def check(self, name, got, ref, mask=None, sentinel=None):
        got = np.asarray(got, F8).reshape(-1)
        v, e = (np.asarray(t, F8).reshape(-1) for t in split(ref))
        assert got.shape == v.shape, "%s %s: shape %s vs %s" % (self.what, name, got.shape, v.shape)
        if mask is not None:
            keep = np.asarray(mask).reshape(-1)
            if sentinel is not None:
                stray = np.flatnonzero(~keep & (got != F8(sentinel)))
                if stray.size:
                    self.bad.append("%s: %d elements outside what the header says is written lost the sentinel (first at %d: %.9g)"
                                    % (name, stray.size, stray[0], got[stray[0]]))
            idx = np.flatnonzero(keep)
            got, v, e = got[idx], v[idx], e[idx]
        else:
            idx = np.arange(got.size)
        if not np.isfinite(got).all():
            self.bad.append("%s: %d non-finite outputs (first at %d)" % (name, int((~np.isfinite(got)).sum()), idx[np.argmax(~np.isfinite(got))]))
            return
        assert np.isfinite(v).all() and np.isfinite(e).all(), "%s %s: the helper is wrong (non-finite reference or bound)" % (self.what, name)
        err = np.abs(got - v)
        dead = e == 0
        if np.any(err[dead] != 0):
            j = np.flatnonzero(dead & (err != 0))
            self.bad.append("%s: %d of %d elements whose bound is zero are not exact (first at %d: got %.9g, want %.9g)"
                            % (name, j.size, int(dead.sum()), idx[j[0]], got[j[0]], v[j[0]]))
        live = ~dead
        if live.any():
            q = err[live] / e[live]
            j = int(np.argmax(q))
            if q[j] > self.worst:
                self.worst, self.where = float(q[j]), "%s[%d]" % (name, idx[np.flatnonzero(live)[j]])
            if q[j] > 1.0:
                k = np.flatnonzero(live)[j]
                self.bad.append("%s: %d of %d elements outside the bound; worst element %d: got %.9g, float64 %.9g, err / bound %.3f"
                                % (name, int((q > 1).sum()), int(live.sum()), idx[k], got[k], v[k], q[j]))
        self.n += got.size

    def line(self, amb=0):
        return "%s: worst err / bound %.3f at %s; %d elements; %d ambiguous rows" % (self.what, self.worst, self.where or "-", self.n, amb)

    def finish(self, amb=0, quiet=False):
        if not quiet:
            print(self.line(amb))
        assert not self.bad, "%s:\n  %s" % (self.what, "\n  ".join(self.bad))
        return self.worst


def check_loss(case, got, ref, what, stats=True, grad=True, quiet=False):
    """got: dict of arrays as a launch (or an X32 emulation) left them; ref: run_loss(case, XVE, ...).  Checks every stored element."""
    rep = Report(what)
    ml, mv = written(case)
    if grad:
        rep.check("dlogits", got["dlogits"], ref["dlogits"], ml, SENT)
        rep.check("dvalues", got["dvalues"], ref["dvalues"], mv, SENT)
    for name in ("losses", "demo_losses"):
        if name in ref:
            v = np.array([split(t)[0] for t in ref[name]])
            e = np.array([split(t)[1] for t in ref[name]])
            rep.check(name, np.asarray(got[name], F8)[:len(ref[name])], VE(v, e))
    for name in ("stats", "demo_stats"):
        if stats and name in ref:
            v = np.stack([split(t)[0] for t in ref[name]], 1)                         # [2][6]
            e = np.stack([split(t)[1] for t in ref[name]], 1)
            rep.check(name, np.asarray(got[name], F8)[:, :6], VE(v, e))
    n_amb = int((ref["amb"] & ~case.planted).sum())
    rep.finish(n_amb, quiet)
    return rep.worst, n_amb


def emulate_loss(case, order="tree", mut=(), **kw):
    """The X32 emulation's outputs in the layout check_loss takes."""
    o = run_loss(case, X32(order), mut=mut, **kw)
    out = dict(dlogits=o["dlogits"], dvalues=o["dvalues"])
    for name in ("losses", "demo_losses"):
        if name in o:
            out[name] = np.array([float(t) for t in o[name]])
    for name in ("stats", "demo_stats"):
        if name in o:
            out[name] = np.stack([np.asarray(t, F8) for t in o[name]], 1)
    return out


# ----------------------------------------------------------------------------- the front kernels
def front_reference(x, rk):
    """raw fp32 [R][K] -> pairs (lg, pk [R][K], H [R]) and the XVE namespace (amb)."""
    X = XVE(x.shape[0])
    lg, pk, H, _s, _t = front(X, X.c(x), rk)
    return X, lg, pk, H


def candidates(score):
    """bool [R][K]: the bins that the error bounds cannot tell from the largest score (the argmax itself included)."""
    n = np.arange(score.v.shape[0])
    top = np.argmax(score.v, -1)
    return (score.v[n, top][:, None] - score.v) <= (score.e[n, top][:, None] + score.e)


# ----------------------------------------------------------------------------- clip + Adam
ADAM = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)
SEG_SIZES = (1000, 257, 4096, 33, 4, 0)


def adam_hp(step, max_norm, lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"]):
    """The fp32 scalars as cadre_clip_adam forms them on the host (cadre_kernels.hip) — the graph forms compute the same two doubles on
    the device."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return (F4(max_norm), F4(lr / bc1), F4(1.0 - beta1), F4(beta2), F4(1.0 - beta2), F4(math.sqrt(bc2)), F4(eps))


class AdamCase:
    """An arena of contiguous segments of SEG_SIZES elements — aligned: every segment padded with zeros (parameter, gradient, moments) to a
    multiple of 4 elements, as the arena lays them out; otherwise the offsets are the running sums, no multiples of 4 — and three
    gradients log-uniform in magnitude from 1e-10 to 1e2 with random sign, times per-segment scales so that the clip bites in some
    segments and not in others.  warm: non-zero starting moments."""

    def __init__(self, seed, sizes=SEG_SIZES, aligned=True, warm=False, max_norm=250.0):
        r = np.random.RandomState(seed)
        lens = [n + (-n % 4 if aligned else 0) for n in sizes]
        self.seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.n, self.max_norm, self.sizes = int(self.seg_off[-1]), max_norm, sizes
        live = np.zeros(self.n, bool)
        for a, n in zip(self.seg_off[:-1], sizes):
            live[a:a + n] = True
        scale = np.repeat(np.array([1.0, 1e-4, 30.0, 1e-2, 1.0, 1.0])[:len(sizes)], lens)
        self.p0 = np.where(live, r.standard_normal(self.n), 0).astype(F4)
        self.m0 = np.where(live & warm, up.log_uniform(r, self.n, -6, 0), 0).astype(F4)
        self.v0 = np.where(live & warm, np.abs(up.log_uniform(r, self.n, -12, 0)), 0).astype(F4)
        self.grads = [np.where(live, up.log_uniform(r, self.n, -10, 2) * scale, 0).astype(F4) for _ in range(3)]

    def segs(self, rlo=0, rhi=None):
        rhi = self.n if rhi is None else rhi
        return [(max(int(a), rlo), min(int(b), rhi)) for a, b in zip(self.seg_off[:-1], self.seg_off[1:])]


def norms2_ref(g, seg_off, rlo=0, rhi=None):
    """float64 sum of squares per segment (math.fsum: exact to the last bit) and the bound of any order of double additions."""
    rhi = g.size if rhi is None else rhi
    v, e = [], []
    for a, b in zip(seg_off[:-1], seg_off[1:]):
        a, b = max(int(a), rlo), min(int(b), rhi)
        s = math.fsum((g[a:b].astype(F8) ** 2).tolist()) if b > a else 0.0
        v.append(s)
        e.append((b - a + 8) * 2.0 ** -53 * s if b > a else 0.0)
    return VE(np.array(v), np.array(e))


def adam_step(case, X, step, p, g, m, v, norms2, rlo=0, rhi=None, mut=()):
    """One clip + Adam step on elements [rlo, rhi) of the arena in the arithmetic of X from the fp32 state (p, m, v: whole-arena arrays;
    norms2: the per-segment square norms AS STORED) -> (p', m', v') typed whole-arena; elements outside the range keep (value, 0)."""
    hp = adam_hp(step, case.max_norm)
    pair = X is XVE
    if pair:
        # step_size = (float)(lr / bc1) and bc2_sqrt = (float)sqrt(bc2) are formed on the host by cadre_clip_adam and on the device by the
        # graph forms: pow() of another library may leave the double an ulp apart, so the fp32 number is one rounding of ALMOST that double
        d = [ADAM["lr"] / (1.0 - ADAM["beta1"] ** step), math.sqrt(1.0 - ADAM["beta2"] ** step)]
        hp = (hp[0], VE(d[0], (U + 1e-14) * d[0])) + hp[2:5] + (VE(d[1], (U + 1e-14) * d[1]), hp[6])
    outs = [VE(a.astype(F8)) for a in (p, m, v)] if pair else [np.array(a, dtype=X.dtype) for a in (p, m, v)]
    for i, (a, b) in enumerate(case.segs(rlo, rhi)):
        if b <= a:
            continue
        x_ = XVE(b - a) if pair else X
        c = x_.c if pair else (lambda t: np.asarray(t, x_.dtype))
        res = adam_row(x_, c(p[a:b]), c(g[a:b]), c(m[a:b]), c(v[a:b]), math.sqrt(float(norms2[i])), hp, mut)
        for o, r_ in zip(outs, res):
            rv, re = split(r_)
            if pair:
                o.v[a:b], o.e[a:b] = rv, re
            else:
                o[a:b] = rv
    return outs


def old_metric(got, ref):
    """max|got - ref| / max|ref|: the metric of the loss tests this file goes beyond (bar 2e-5)."""
    got, ref = np.asarray(got, F8), np.asarray(ref, F8)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


# ----------------------------------------------------------------------------- the cases (shared by the CPU and the GPU file)
# B 1 / 15 / 16 / 17 / 33 / 200 (one row; one short of, exactly, one past a workgroup's 16 rows; a third workgroup with one row; 13
# workgroups), (K_steer, K_throttle) (33, 3) / (64, 2) / (1, 64), C 1 / 4 / 6, pitch 64 and 40 (K < ldl < 64), logit scales 1 / 4 / 16, both
# heads categorical / both ordinal / one of each, clip 0.125 (the planted max tie outside the clamp), clip 0 (the planted ratio on the
# clamp), ent_coeff 0.  Seeds: chosen so that the float64 pairs alone meet at most one ambiguous row (tests/test_loss_parity_cpu.py).
PPO_CASES = [
    dict(seed=11, B=1, Ks=(33, 3), C=1, ldl=64, scale=1.0),
    dict(seed=12, B=15, Ks=(33, 3), C=4, ldl=40, scale=4.0),
    dict(seed=13, B=16, Ks=(64, 2), C=6, ldl=64, scale=16.0),
    dict(seed=14, B=17, Ks=(1, 64), C=4, ldl=64, scale=1.0, clip=0.125, ent_coeff=0.0),
    dict(seed=15, B=15, Ks=(1, 64), C=1, ldl=64, scale=4.0, clip=0.0),
    dict(seed=16, B=33, Ks=(33, 3), C=4, ldl=40, scale=4.0, ordinal=(True, True)),
    dict(seed=17, B=200, Ks=(33, 3), C=4, ldl=64, scale=16.0, clip=0.25),
    dict(seed=18, B=33, Ks=(64, 2), C=6, ldl=64, scale=1.0, ordinal=(True, False)),
    dict(seed=19, B=17, Ks=(33, 3), C=1, ldl=40, scale=16.0, ordinal=(False, True)),
    dict(seed=20, B=200, Ks=(33, 3), C=4, ldl=64, scale=1.0, ordinal=(True, True)),
]
BC_CASES = [
    dict(seed=31, B=1, Ks=(33, 3), C=1, ldl=64, scale=1.0, smoothing=0.1),
    dict(seed=32, B=17, Ks=(33, 3), C=4, ldl=40, scale=4.0, smoothing=0.1),
    dict(seed=33, B=33, Ks=(64, 2), C=6, ldl=64, scale=1.0, smoothing=0.0, ordinal=(True, True)),
    dict(seed=34, B=16, Ks=(1, 64), C=1, ldl=64, scale=16.0, smoothing=0.0, ordinal=(False, True)),
    dict(seed=35, B=200, Ks=(33, 3), C=4, ldl=64, scale=16.0, smoothing=0.1),
    dict(seed=36, B=15, Ks=(33, 3), C=4, ldl=40, scale=4.0, smoothing=0.1, ordinal=(True, False)),
]
MIX_CASES = [
    dict(seed=51, B=33, Ks=(33, 3), C=4, ldl=40, scale=4.0),
    dict(seed=52, B=200, Ks=(33, 3), C=4, ldl=64, scale=1.0, ordinal=(True, True), smoothing=0.0),
    dict(seed=53, B=17, Ks=(64, 2), C=6, ldl=64, scale=16.0, ordinal=(False, True), empty="no_ppo_head0"),
    dict(seed=54, B=16, Ks=(1, 64), C=1, ldl=64, scale=1.0, empty="no_demo_head1", clip=0.125),
    dict(seed=55, B=15, Ks=(33, 3), C=4, ldl=40, scale=16.0, ordinal=(True, False)),
]


def loss_cases(kind):
    return [LossCase(kind=kind, **kw) for kw in dict(ppo=PPO_CASES, bc=BC_CASES, mix=MIX_CASES)[kind]]


def branches(case):
    """(rows clipped above, clipped below, unclipped) among the PPO rows of the case, from float64."""
    X, n = X64(), [0, 0, 0]
    for h in range(2):
        rows = case.rows(h, False)
        if rows.size == 0 or case.kind == "bc":
            continue
        lg = front(X, case.own_logits(h, rows).astype(F8), case.rk(h))[0]
        ratio = np.exp(lg[np.arange(rows.size), case.actions[h, rows]] - case.old_lp[h, rows])
        c = float(case.hp["clip"])
        n[0] += int((ratio > 1 + c).sum())
        n[1] += int((ratio < 1 - c).sum())
        n[2] += int(((ratio >= 1 - c) & (ratio <= 1 + c)).sum())
    return tuple(n)
