"""Element-wise float64 parity bound for the attention kernels — the bound, stated once ("attention parity").  The kernels
(cadre_kernels.hip): position attention pam_kernel / pam_large_kernel (cadre_pam, cadre_pam_bf16out), channel attention cam_kernel /
cam_large_kernel / cam_split_kernel (cadre_cam, cadre_cam_bf16out) and the inter-task tail intertask_kernel (cadre_intertask_att).

The test is

    |got - y64|  <=  err64        for EVERY stored element,

no factor on the total, no sampled subset, no exempt share; every checked output is finite; an element whose bound is zero must be bit-equal
to y64 (an all-zero frame through PAM or CAM, an all-zero position through CAM).  y64 is the float64 evaluation of the kernel's statements
on the operands as stored; err64 is composed of pieces the project already trusts:

    matrix-core product of STORED fp32 operands (PAM q k^T, K = 16; CAM x^T x, K = Np)
        c_bar 2^-24 mag, mag = sum |a||b| (tests/f32_parity.py).  c_bar is obtained as f32_parity.c_bar_direct obtains it: the case's own
        products, rounded to fp32 and summed strictly sequentially (ascending k) on the CPU, the worst error over float64 in units of
        2^-24 mag over ALL outputs of the frame, doubled (f32_parity.FACTOR) and asserted under DIRECT_CAP(K) = K + 5.  It is never taken
        from a kernel.  The maximum over a handful of chains is no estimate of a chain's worst: a frame with fewer than MIN_CHAINS = 1024
        chains of non-zero magnitude takes the a-priori cap itself.
    the softmax statements up to e = expf(t - mx)
        the energies enter as (value, error) pairs of tests/loss_parity.py (XVE): every operation adds half an fp32 ulp of its result and
        propagates its operands' errors to first order, exp multiplies the incoming error by the result and adds T_EXP = update_parity.T_EXP
        ulps plus the 2^-126 floor.  A padding column enters as -inf and leaves expf as an exact zero.  The maximum is X.max (the largest
        error of its operands); where it is the shift a softmax subtracts (PAM's mx, CAM's rowmax and m2, the inter-task mx) its error is
        dropped: e / s is the same real number for every shift, and the kernel's maximum is one (_shift).
    the sum, the divide and the second product (PAM att v, K = Np; CAM x att^T, K = 128), composed together (attend)
        o = sum_d w_d e_d / sum_d e_d is a weighted mean, so an error d e_d of a numerator moves it by (w_d - o) d e_d / s to first order:
        the propagated part is sum_d |w_d - o| |d e_d| / s (the float64 matrix products |d att| @ |v| and |x| @ |d att|^T with the
        mean's own cancellation kept: |d att| formed element by element counts every d e_d once in its numerator and again, with the
        sign it cannot have, in every denominator — twice the error on near-uniform rows, which alone puts a 128-position CAM frame
        above the old bar's tolerance).  The row sum (a lane's strided partial sum of n_strided terms, then the 6-deep shuffle tree:
        (n_strided - 1) + 6 roundings) and the one divide per element change att_d by a factor 1 + u_d - sigma: (n_strided + 6) 2^-24
        (|att| @ |w|).  The chain's own part is c_bar2 2^-24 (|att| @ |w|), c_bar2 measured as c_bar above on the fp32 attention of this
        module's emulation, doubled and capped by DIRECT_CAP(K).
    the epilogue gamma * o + x
        two pair operations; a contraction into one fma rounds once and is covered.
    the inter-task chains (sum += e; o += V[j] * e over j = 0 .. 255, strictly sequential)
        counted from the code: the first addition is 0 + term (exact), the other 255 each round the partial sum S_j they produce:
        2^-24 sum_{j = 1..255} |S_j|; `o` adds one rounding per product V[j] * e (256; none if the compiler fuses — covered).  q / temp,
        q k - mx (two roundings; one under fma), expf, the divide and + V[i] are pair operations.

The only non-smooth operation is the maximum (Lipschitz with constant one: X.max; fmaxf of the two candidate row maxima of the inter-task
kernel goes through X.fmax, which would mark a row ambiguous if an unsure comparison chose between values further apart than their
bounds).  No case may produce an ambiguous row: asserted from the pairs (reference()).

Each kernel's body is written ONCE (pam_row, cam_row, intertask_row), generic over the operand namespace: X64 (the reference), XVE (the
bound), X32 (the fp32 emulation: order "tree" = the kernels' order — ascending k chains, strided lane sums and the shuffle tree —, order
"seq" = strictly sequential row sums and the chains the other way round, k descending).  `mut` names one-statement mutants.

Plain helper module (no GPU, no fixtures)."""
import functools
import zlib

import numpy as np

from tests import f32_parity as fp
from tests import loss_parity as lp
from tests.loss_parity import F4, F8, U, VE, X32, X64, XVE, Report, split  # noqa: F401

T_EXP = lp.T_EXP
MIN_CHAINS = 1024
SENT = F4(-7.5)
GAMMA_PAM, GAMMA_CAM = F4(0.5), F4(0.7)
NEG_INF = -np.inf

PAM_SIZES = (1, 2, 3, 31, 32, 33, 40, 64, 65, 81, 127, 128, 129, 1024)
CAM_SIZES = (1, 2, 3, 31, 32, 33, 40, 64, 65, 81, 127, 128, 129, 144)
BIG = 1024
FAMILIES = ("benign", "peaked", "offset", "relu", "zero")
TRIPLES = (("benign", "peaked", "offset"), ("relu", "zero", "offset"))        # F = 3 frames of different families; both cover all five
OLD_SIZES = (9, 40, 81, 110, 121, 128, 144, 143, 256, 500)                  # h * w of test_kernels_gpu.py::test_pam_cam
IT_FAMILIES = ("benign", "large", "equal_keys", "zero_query")
TEMPS = (16.0, 10.0)

PAM_MUTANTS = ("pam_last_key_dropped", "pad_exp0", "att_transposed", "no_max", "k_step_left_out", "gamma_on_residual", "prev_frame_residual")
CAM_MUTANTS = ("pad_row_copies_last", "cam_plain_energy", "att_transposed", "no_max", "k_step_left_out", "gamma_on_residual",
               "prev_frame_residual")
IT_MUTANTS = ("kmax_only", "no_v", "halves_exchanged", "q_times_temp")


# ----------------------------------------------------------------------------- operations the bodies need beyond loss_parity's
def _ve(X):
    return isinstance(X, XVE)


def _T(a):
    return VE(a.v.T, a.e.T) if isinstance(a, VE) else a.T


def _cat(a, b):
    if isinstance(a, VE):
        return VE(np.concatenate([a.v, b.v], -1), np.concatenate([a.e, b.e], -1))
    return np.concatenate([a, b], -1)


def _rows(a, sl):
    return VE(a.v[sl], a.e[sl]) if isinstance(a, VE) else a[sl]


def _const(X, shape, value):
    return X.c(np.full(shape, value))


def _exp(X, a):
    """expf; a -inf operand (a padding column) gives an exact zero whatever the error of the subtracted maximum."""
    p = X.exp(a)
    if isinstance(p, VE):
        dead = a.v == NEG_INF
        return VE(np.where(dead, 0.0, p.v), np.where(dead, 0.0, p.e))
    return p


def _shift(mx):
    """The maximum a softmax subtracts, as the kernel holds it: its error is dropped.  A softmax row is invariant under a common shift of
    its arguments — e / s with e = expf(t - mx) is the same real number for every mx —, the fp32 maximum is one such mx (the maximum of the
    fp32 arguments, taken without rounding; max(t + c) = max(t) + c), and the roundings that follow are relative ones.  CAM's row maximum
    in rowmax - E is the same kind of shift."""
    return VE(mx.v, 0.0) if isinstance(mx, VE) else mx


def _sub(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return a - b


def chain32(a, b, ks):
    """fp32 [N][K] x [K][M]: every product rounded to fp32, added to the running sum in the order ks."""
    acc = np.zeros((a.shape[0], b.shape[1]), F4)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in ks:
            acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    assert acc.dtype == F4
    return acc


def prod_k(X, a, b, cb=None, drop=()):
    """sum_k a[n][k] b[k][m], the matrix-core fma chain in ascending k.  drop: k indices a mutant leaves out."""
    K = a.shape[1]
    ks = [k for k in range(K) if k not in drop]
    if _ve(X):
        v = a.v[:, ks] @ b.v[ks]
        mag = np.abs(a.v[:, ks]) @ np.abs(b.v[ks])
        return VE(v, a.e[:, ks] @ np.abs(b.v[ks]) + np.abs(a.v[:, ks]) @ b.e[ks] + a.e[:, ks] @ b.e[ks] + cb * U * mag)
    if X.dtype is F8:
        return a[:, ks] @ b[ks]
    return chain32(a, b, ks if X.order == "tree" else ks[::-1])


def lane_sum(X, p):
    """A wave's sum of a row [rows][R]: lane l adds columns l, l + 64, .. in turn (s = 0; s += e: the first addition is exact), then
    the 6-deep xor-shuffle tree."""
    if _ve(X):
        n_str = -(-p.v.shape[-1] // 64)
        exact = lp._int_sum(p, -1)
        return VE(p.v.sum(-1), p.e.sum(-1) + np.where(exact, 0.0, (n_str - 1 + 6) * U * np.abs(p.v).sum(-1)))
    if X.dtype is F8:
        return p.sum(-1)
    if X.order == "seq":
        return np.cumsum(p, -1, dtype=F4)[..., -1]
    R = p.shape[-1]
    pad = -R % 64
    if pad:
        p = np.concatenate([p, np.zeros(p.shape[:-1] + (pad,), F4)], -1)
    lanes = np.cumsum(p.reshape(p.shape[:-1] + (-1, 64)), -2, dtype=F4)[..., -1, :]
    return X.sum(lanes)


def seq_sum(X, a):
    """A strictly sequential sum over the last axis, j ascending from a zero accumulator."""
    if _ve(X):
        S = np.cumsum(a.v, -1)
        exact = lp._int_sum(a, -1)
        return VE(S[..., -1], a.e.sum(-1) + np.where(exact, 0.0, U * np.abs(S[..., 1:]).sum(-1)))
    if X.dtype is F8:
        return a.sum(-1)
    if X.order == "seq":
        a = a[..., ::-1]
    return np.cumsum(a, -1, dtype=F4)[..., -1]


def softmax_rows(X, t, mut=()):
    """The kernels' row softmax on [rows][R]: mx = max, e = expf(t - mx), s = the lane sum, e / s (one divide per element).
    -> (attention, e, s)."""
    if "no_max" in mut:
        p = _exp(X, t)
    else:
        mx = _shift(X.max(t))
        p = _exp(X, _sub(t, mx[..., None]))
    s = lane_sum(X, p)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return p / s[..., None], p, s


def attend(X, t, w, left, ncols, aux, mut=(), drop=()):
    """The row softmax of t [rows][R] (columns >= ncols are padding) and the product that follows it.  left: o[n][c] = sum_m att[n][m]
    w[m][c] (PAM: w = v); otherwise o[n][c] = sum_d w[n][d] att[c][d] (CAM: w = x).  The bound of the pair (softmax, product) is composed
    here, see the module docstring; the emulation leaves its attention in aux["att"]."""
    cols = (slice(None), slice(0, ncols))
    att, p, s = softmax_rows(X, t, mut)
    att = _rows(att, cols)
    if "att_transposed" in mut:
        att = _T(att)
    if not _ve(X):
        aux["att"] = att
        aux["o"] = prod_k(X, att, w, None, drop) if left else prod_k(X, w, _T(att))
        return aux["o"]
    n_str = -(-t.v.shape[-1] // 64)
    sv, wv = p.v.sum(-1), w.v
    assert (w.e == 0).all()
    a64 = p.v[cols] / sv[:, None]
    q = p.e[cols] / sv[:, None]                                                  # |d e| / s
    o = a64 @ wv if left else wv @ a64.T
    absw = a64 @ np.abs(wv) if left else np.abs(wv) @ a64.T
    spread = np.zeros_like(o)
    step = max(1, (1 << 22) // (a64.shape[1] * wv.shape[1]))
    for i in range(0, o.shape[0], step):
        sl = slice(i, i + step)
        if left:                                                                 # sum_m q[n][m] |w[m][c] - o[n][c]|
            spread[sl] = (np.abs(wv[None, :, :] - o[sl, None, :]) * q[sl, :, None]).sum(1)
        else:                                                                    # sum_d q[c][d] |w[n][d] - o[n][c]|
            spread[sl] = (np.abs(wv[sl, None, :] - o[sl, :, None]) * q[None, :, :]).sum(2)
    return VE(o, spread + (n_str + 6 + aux["cb_o"]) * U * absw)


# ----------------------------------------------------------------------------- the bodies, each written once
def pam_row(X, q, k, v, x, gamma, aux, mut=(), x_res=None):
    """One frame of pam_large_kernel / pam_kernel.  q, k [Np][16], v, x [Np][128] typed by X; gamma an fp32 number.  aux: c_bar values
    ("cb_e", "cb_o") for XVE; the emulation leaves its attention in aux["att"].  x_res: the residual a mutant reads instead of x."""
    Np = q.shape[0]
    R = 32 * ((Np + 31) // 32)
    drop = (6, 7) if "k_step_left_out" in mut else ()
    e = prod_k(X, q, _T(k), aux.get("cb_e"), drop)                               # e[n][m] = sum_k q[n][k] k[m][k]
    if "att_transposed" in mut:
        e = _T(e)
    if R > Np:                                                                   # columns m >= Np: -inf before the softmax
        e = _cat(e, _const(X, (Np, R - Np), 0.0 if "pad_exp0" in mut else NEG_INF))
    drop2 = (Np - 1,) if "pam_last_key_dropped" in mut and Np > 1 else ()
    o = attend(X, e, v, True, Np, aux, mut, drop2)                               # row softmax; o[n][c] = sum_m att[n][m] v[m][c]
    return _epilogue(X, o, x, gamma, mut, x_res)


def cam_row(X, x, gamma, aux, mut=(), x_res=None):
    """One frame of cam_split_kernel / cam_large_kernel / cam_kernel.  x [Np][128] typed by X."""
    Np = x.shape[0]
    xe = x
    if Np % 2 and "pad_row_copies_last" in mut:                                  # the k pair's second row when Np is odd: zero
        xe = VE(np.concatenate([x.v, x.v[-1:]]), np.concatenate([x.e, x.e[-1:]])) if isinstance(x, VE) else np.concatenate([x, x[-1:]])
    drop = (2 * (Np // 4), 2 * (Np // 4) + 1) if "k_step_left_out" in mut and Np >= 2 else ()
    E = prod_k(X, _T(xe), xe, aux.get("cb_e"), drop)                             # E[c][d] = sum_n x[n][c] x[n][d]
    if "cam_plain_energy" in mut:
        n = E
    else:
        n = _sub(_shift(X.max(E))[..., None], E)                                 # rowmax - E
    o = attend(X, n, x, False, 128, aux, mut)                                    # m2 = max n, p = expf(n - m2), s, p / s; o[n][c] = sum_d x[n][d] att[c][d]
    return _epilogue(X, o, x, gamma, mut, x_res)


def _epilogue(X, o, x, gamma, mut, x_res):
    g = X.c(F4(gamma))
    r = x if x_res is None else x_res
    with np.errstate(invalid="ignore", over="ignore"):
        if "gamma_on_residual" in mut:
            return g * (o + r)
        return g * o + r


def intertask_row(X, Q, K, V, temp, mut=()):
    """One direction of one frame of intertask_kernel: Q, K, V [256] typed by X -> [256]."""
    t = X.c(F4(temp))
    qi = Q * t if "q_times_temp" in mut else Q / t
    kv = split(K)[0]
    kmax, kmin = X.c(kv.max()), X.c(kv.min())                                    # extremes of stored numbers: exact
    a, b = qi * kmax, qi * kmin
    mx = _shift(a if "kmax_only" in mut else X.fmax(a, b))
    with np.errstate(invalid="ignore", over="ignore"):
        e = _exp(X, qi[:, None] * K[None, :] - mx[:, None])                      # e_j = expf(qi * K[j] - mx)
        sm = seq_sum(X, e)
        o = seq_sum(X, V[None, :] * e)
        r = o / sm
        return r if "no_v" in mut else r + V


# ----------------------------------------------------------------------------- c_bar of a matrix-core product
def c_bar_chain(a, b, K, what="", chain=None):
    """a [N][K], b [K][M]: the fp32 operands of one frame's product -> (c_bar, cap, chains).  The sequential fp32 chain (products rounded,
    ascending k), the worst error over float64 in units of 2^-24 mag over every output whose magnitude is not zero, doubled; the cap
    itself where fewer than MIN_CHAINS chains were summed.  chain: chain32(a, b, ascending k) where the emulation has formed it already."""
    cap = float(fp.DIRECT_CAP(K))
    assert a.dtype == F4 and b.dtype == F4 and a.shape[1] <= K
    y = a.astype(F8) @ b.astype(F8)
    mag = np.abs(a.astype(F8)) @ np.abs(b.astype(F8))
    live = mag > 0
    worst, chains = 0.0, int(live.sum())
    if chains:
        err = np.abs((chain32(a, b, range(a.shape[1])) if chain is None else chain).astype(F8) - y)
        worst = float((err[live] / (U * mag[live])).max())
    c_bar = fp.FACTOR * worst
    assert c_bar <= cap, "%s: c_bar %.3g above the cap %g: the helper is wrong" % (what, c_bar, cap)
    return (c_bar if chains >= MIN_CHAINS else cap), cap, chains


# ----------------------------------------------------------------------------- input families (seeded)
def _rs(*key):
    return np.random.RandomState(zlib.crc32(" ".join(str(k) for k in key).encode()))


def _relu_frame(r, Np):
    x = np.maximum(0.0, 0.4 * r.standard_normal((Np, 128)))
    x[:, [5, 64, 127]] = 0.0                                                     # channels identically zero
    x[Np // 2, :] = 0.0                                                          # one position identically zero
    return x


def pam_frame(family, Np, slot):
    """-> (x [Np][128], qkv [Np][160]) fp32.  qkv is the fp32 rounding of the float64 projection x W^T + b (q 16 | k 16 | v 128), then
    edited per family; `slot` is the frame's index in its case."""
    r = _rs("pam", family, Np, slot)
    if family == "zero":
        return np.zeros((Np, 128), F4), np.zeros((Np, 160), F4)
    x = _relu_frame(r, Np) if family == "relu" else 0.4 * r.standard_normal((Np, 128))
    x = x.astype(F4)
    W, b = 0.1 * r.standard_normal((160, 128)), 0.1 * r.standard_normal(160)
    qkv = x.astype(F8) @ W.T + b
    if family == "peaked":                                                       # a few query rows aligned with one key: energies 32 .. 80 apart
        u = r.standard_normal(16)
        u /= np.linalg.norm(u)
        ms = r.randint(Np)
        qkv[ms, 16:32] = 8.0 * u
        for i, n in enumerate(sorted(set(r.randint(Np, size=min(Np, 5)).tolist()))):
            qkv[n, 0:16] = (4.0 + 1.5 * i) * u
    elif family == "offset":                                                     # q . k around +200, nearly equal: 16 * 3.5^2 = 196
        qkv[:, 0:32] += 3.5
    return x, qkv.astype(F4)


def cam_frame(family, Np, slot):
    r = _rs("cam", family, Np, slot)
    if family == "zero":
        return np.zeros((Np, 128), F4)
    if family == "relu":
        return _relu_frame(r, Np).astype(F4)
    x = 0.4 * r.standard_normal((Np, 128))
    if family == "peaked":
        x[:, 37] *= 10.0
    elif family == "offset":
        x = 1.5 + 0.05 * r.standard_normal((Np, 128))
    return x.astype(F4)


def intertask_frame(family, temp, slot):
    """-> [6][256] fp32: visual q, k, v, bc q, k, v."""
    r = _rs("it", family, temp, slot)
    a = 2.0 * r.standard_normal((6, 256))
    if family == "large":                                                        # |q||k| / temp up to about 200, q of both signs
        sd = np.sqrt(200.0 * temp) / 3.0
        a[[0, 1, 3, 4]] = sd * np.clip(r.standard_normal((4, 256)), -3.0, 3.0)
    elif family == "equal_keys":
        a[1, :], a[4, :] = a[1, 0], a[4, 0]
    a = a.astype(F4)
    if family == "zero_query":
        a[0, 5] = a[3, 5] = F4(0.0)
        a[0, 9] = a[3, 9] = F4(-0.0)
    return a


# ----------------------------------------------------------------------------- cases
class AttCase:
    """F frames of one size, each of its own family, as the kernels address them: x [F][Np][128], qkv [F][Np][160] (PAM)."""

    def __init__(self, kind, Np, fams):
        self.kind, self.Np, self.fams, self.F = kind, Np, tuple(fams), len(fams)
        self.gamma = GAMMA_PAM if kind == "pam" else GAMMA_CAM
        if kind == "pam":
            fr = [pam_frame(f, Np, i) for i, f in enumerate(fams)]
            self.x, self.qkv = np.stack([a for a, _ in fr]), np.stack([b for _, b in fr])
        else:
            self.x, self.qkv = np.stack([cam_frame(f, Np, i) for i, f in enumerate(fams)]), None

    def tag(self):
        return "%s Np %d frames %s" % (self.kind, self.Np, "/".join(self.fams))


def run_att(case, X, aux=None, mut=()):
    """All frames of a case in the arithmetic of X -> typed [F][Np][128] (a VE for XVE).  aux: c_bar values in, the attention of every
    frame out (aux["att"]: list)."""
    aux = {} if aux is None else aux
    c = X.c if _ve(X) else (lambda a: np.asarray(a, X.dtype))
    outs, atts, prods = [], [], []
    for f in range(case.F):
        x = c(case.x[f])
        x_res = c(case.x[max(f - 1, 0)]) if "prev_frame_residual" in mut else None
        fa = {k: v[f] for k, v in aux.items() if k not in ("att", "o")}
        if case.kind == "pam":
            qkv = case.qkv[f]
            y = pam_row(X, c(qkv[:, 0:16]), c(qkv[:, 16:32]), c(qkv[:, 32:160]), x, case.gamma, fa, mut, x_res)
        else:
            y = cam_row(X, x, case.gamma, fa, mut, x_res)
        outs.append(y)
        atts.append(fa.get("att"))
        prods.append(fa.get("o"))
    aux["att"], aux["o"] = atts, prods
    if _ve(X):
        return VE(np.stack([y.v for y in outs]), np.stack([y.e for y in outs]))
    return np.stack(outs)


def reference(case):
    """-> dict(y = the pairs [F][Np][128], emu = the "tree" emulation's fp32 result, cb = per product the (c_bar, cap, chains) of every frame)."""
    aux32 = {}
    emu = run_att(case, X32("tree"), aux32)
    if case.kind == "pam":
        first = [(case.qkv[f][:, 0:16].copy(), case.qkv[f][:, 16:32].T.copy()) for f in range(case.F)]
        second = [(aux32["att"][f], case.qkv[f][:, 32:160].copy()) for f in range(case.F)]
        K1, K2 = 16, case.Np
    else:
        first = [(case.x[f].T.copy(), case.x[f]) for f in range(case.F)]
        second = [(case.x[f], aux32["att"][f].T.copy()) for f in range(case.F)]
        K1, K2 = case.Np, 128
    cb_e = [c_bar_chain(a, b, K1, "%s frame %d energy" % (case.tag(), f)) for f, (a, b) in enumerate(first)]
    cb_o = [c_bar_chain(a, b, K2, "%s frame %d product" % (case.tag(), f), aux32["o"][f]) for f, (a, b) in enumerate(second)]
    X = XVE(1)
    y = run_att(case, X, dict(cb_e=[c[0] for c in cb_e], cb_o=[c[0] for c in cb_o]))
    assert not X.amb.any(), "%s: an ambiguous row" % case.tag()
    assert np.isfinite(y.v).all() and np.isfinite(y.e).all(), "%s: the helper is wrong (non-finite reference or bound)" % case.tag()
    return dict(y=y, emu=emu, cb=dict(energy=cb_e, product=cb_o))


@functools.lru_cache(maxsize=None)
def att_case(kind, Np, fams):
    """(case, reference) — computed once, shared by the tests that need it, left unchanged."""
    c = AttCase(kind, Np, fams)
    return c, reference(c)


def case_keys(kind, small_only=False):
    """Every (kind, Np, families) of the GPU file: F = 3 frames of different families at every size, F = 1 at the largest."""
    keys = []
    for Np in (PAM_SIZES if kind == "pam" else CAM_SIZES):
        if Np == BIG:
            if not small_only:
                keys += [(kind, Np, (f,)) for f in FAMILIES]
        else:
            keys += [(kind, Np, t) for t in TRIPLES]
    if kind == "cam" and not small_only:
        keys.append((kind, BIG, ("benign",)))
    return keys


def check_att(got, ref, what, quiet=False):
    """got [F][Np][128] against the pairs; -> worst err / bound."""
    rep = Report(what)
    rep.check("y", got, ref["y"])
    return rep.finish(0, quiet)


class ItCase:
    """F frames of inter-task operands qkv [F][6][256], each frame of its own family."""

    def __init__(self, fams, temp):
        self.fams, self.F, self.temp = tuple(fams), len(fams), float(temp)
        self.qkv = np.stack([intertask_frame(f, temp, i) for i, f in enumerate(fams)])

    def tag(self):
        return "intertask F %d temp %g frames %s" % (self.F, self.temp, "/".join(self.fams))


def run_it(case, X, mut=()):
    """-> typed [F][512]: [att_visual | att_bc] — direction 1 (bc query x visual key -> visual value) first, then direction 0."""
    c = X.c if _ve(X) else (lambda a: np.asarray(a, X.dtype))
    rows = []
    for f in range(case.F):
        vq, vk, vv, bq, bk, bv = (c(case.qkv[f, i]) for i in range(6))
        d0 = intertask_row(X, vq, bk, bv, case.temp, mut)
        d1 = intertask_row(X, bq, vk, vv, case.temp, mut)
        rows.append(_cat(d0, d1) if "halves_exchanged" in mut else _cat(d1, d0))
    if _ve(X):
        return VE(np.stack([r.v for r in rows]), np.stack([r.e for r in rows]))
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def it_case(fams, temp):
    c = ItCase(fams, temp)
    X = XVE(256)
    y = run_it(c, X)
    assert not X.amb.any(), "%s: an ambiguous row" % c.tag()
    assert np.isfinite(y.v).all() and np.isfinite(y.e).all()
    return c, dict(y=y)


def it_keys():
    return [(IT_FAMILIES, t) for t in TEMPS] + [(("large",), TEMPS[1]), (("benign",), TEMPS[0])]


def old_metric(got, ref):
    """max|got - ref| / max|ref|: the metric of test_pam_cam and test_intertask_tail_and_measurements (bar 2e-5)."""
    return lp.old_metric(got, ref)
