"""Element-wise float64 parity bound for the fp32 (config C2) kernels — the bound, stated once ("fp32 parity").

The kernels read fp32 operands and promise "exact fp32 in another order" (DESIGN 3.2, 3.4): every output element is pinned to

    |got - y64|  <=  c_bar * 2^-24 * mag

against the float64 DIRECT convolution / product of the operands as stored plus the float64 epilogue.  No half-ulp term (the output is
fp32: its one rounding is one of the counted ones), no sampling of the kernel's result, no exempt share; every output is finite.

Direct kernels (cadre_gemm_f32 in all its modes, cadre_splitk_reduce, cadre_conv3x3_ring on fp32 operands, the fp32 fused front).
`mag` is the reference on absolute values, |scale| sum|a||b| + |shift| + |resid| (times the slope where a leaky ReLU took the negative
branch).  `c_bar` comes from bf16_parity.c_bar_of: the case's own products (each ROUNDED to fp32 now) summed strictly sequentially with
np.cumsum, the fp32 epilogue, the worst error over float64 in units, doubled.  The chain is summed for EVERY output the kernel is checked
on while the case has at most DIRECT_BUDGET = 2^28 products (every dense and implicit-conv case, the front, the smaller ring cases);
beyond that for budget / K outputs, half at random and half those that cancel least (chain_outputs).  The error of the chain has a
long tail — an output whose partial sums run to four standard deviations collects many times the typical rounding — and the
maximum over a random 4096 of 27200 outputs misses it: at 200 x 136 x 544 the sample's worst is 2.48 units, the chain's worst over
all outputs 4.60, and cadre_gemm_f32 (4.97 at the output where the chain itself has 4.47) exceeded twice the former.
The a-priori cap that replaces the bf16 module's K + 4:
a term a_k b_k reaches the output through ONE rounding of its product (none under fma) and at most K - 1 additions, whatever the order
(sequential, MFMA chunks, split-K slabs and their reduction: every binary tree over K leaves is at most K - 1 deep), then through at
most four epilogue roundings (scale, shift, residual, slope) and one for the slope's own conversion to fp32: K + 5 factors (1 + d),
|d| <= 2^-24, per term, i.e. (1 + 2^-24)^(K+5) - 1 <= 1.001 (K + 5) 2^-24 for K < 2^13.  (Counting "one rounding per product and one per
add" over the SUM gives 2K; per TERM — and mag is a sum over terms — the product's rounding is met once, so the cap is K + 5, the
tighter of the two.)  DIRECT_CAP(K) = K + 5 is asserted on every c_bar.

Winograd kernels (three-launch form, cadre_winograd_c64, cadre_winograd_in_frag -> cadre_winograd_gemm_out).  The reference VALUE
stays the direct float64 convolution; the RULER is the Winograd magnitude

    mag_w = |scale| * |A^T| ( sum_cin |U| (.) (|B^T| |d| |B|) ) |A|  +  |shift| + |resid|            (float64)

because the transforms cancel: the sums a Winograd kernel forms are 3.5 ... 97 times (median; up to 579) larger than the direct ones.
The matrices are built here, exactly, with fractions.Fraction from the Cook-Toom points DESIGN 3.4 documents (cook_toom): A^T is the
Vandermonde matrix of the points, B^T the transposed inverse of the n x n evaluation matrix with row i multiplied by
N_i = prod_{j != i} (p_i - p_j), G the 3-column evaluation matrix with row i divided by N_i; the test asserts
A^T[(G g G^T) (.) (B^T d B)]A = correlation(d, g) over the rationals.  `U` is the fp32 transform-domain weight AS THE HOST PREPARES IT
(encoder._winograd_u; u_from_frag / u_from_c64 un-permute the two fused layouts to [plane][N][Cin]).  The kernels scale the rows of G
differently (powers of two moved between B^T and G): row_scale fits the diagonal D with U_stored = D (G g G^T) D from the stored U
itself (least squares over row 0, snapped to a small rational, then asserted to reproduce every plane to one fp32 rounding), and
mag_w is formed with |D^-1 U D^-1| against this module's own B^T and A^T.  That is independent of how a kernel splits D^-1 between
its B^T and A^T: a diagonal scaling commutes with taking absolute values.

`c_bar` of a Winograd case is never taken from a kernel: wino_case emulates the form in fp32 numpy on a sample of tiles (all tiles when
the case is small; the four corner tiles, whose last row / column may lie partly outside the map, always) with B^T' = D^-1 B^T, A^T and
the stored U.  ORDERS, the set of emulated orders, stated once: transforms row-first and column-first, times the sum over Cin strictly
sequential and in partial sums of 4, 16 and 32 terms (each partial sum sequential, then added to the running sum: the chains an MFMA
can form).  The worst error over those eight orders in units of 2^-24 mag_w is doubled (FACTOR = 2: the maximum over a sample is a
random quantity, and a kernel may contract a multiply-add the emulation rounds twice).  It is asserted below the a-priori cap
WINO_CAP(Cin, m) = Cin + 4 (m + 2) + 8: per term of mag_w one rounding of U, at most m + 2 roundings in each of the two input-transform
passes (m + 2 products of which the first is not added, m + 1 additions), one for the product and Cin - 1 for the accumulation, m + 2 in
each of the two output-transform passes, and eight for what remains: the coefficients of B^T' and A^T that fp32 does not hold exactly
(one per pass, four passes) and the epilogue (scale, shift, residual) with one to spare; 1.001 covers the second order.

Plain helper module (no GPU, no fixtures): tests/test_f32_parity_cpu.py shows that the bound has teeth, tests/test_f32_parity_gpu.py
applies it to the kernels.  Tensors are torch CPU tensors; activations NHWC, conv weights OIHW.
"""
from fractions import Fraction

import numpy as np
import torch

from tests import bf16_parity as bp
from tests.bf16_parity import U, f64, conv_acc, dense_acc, epilogue, conv_products, dense_products, measure, check, failures, pool_ref  # noqa: F401

FACTOR = 2.0                                                     # c_bar = FACTOR * the worst error of the CPU emulation
DIRECT_BUDGET = 1 << 28                                          # products a direct case's sequential chain may sum (chain_outputs)
ORDERS = [(rows_first, chunk) for rows_first in (True, False) for chunk in (1, 4, 16, 32)]
POINTS = {2: [0, 1, -1], 3: [0, Fraction(3, 4), Fraction(-3, 4), 2], 4: [0, Fraction(3, 4), Fraction(-3, 4), Fraction(3, 2), Fraction(-3, 2)],
          6: [0, Fraction(1, 2), Fraction(-1, 2), 1, -1, 2, -2]}  # + infinity, last


def DIRECT_CAP(K):
    return K + 5


def WINO_CAP(Cin, m):
    return Cin + 4 * (m + 2) + 8


# ----------------------------------------------------------------------------- direct kernels
def epilogue32(acc, mac, scale=None, shift=None, resid=None, act=0, slope=0.01):
    """bf16_parity.epilogue, with the magnitude following a leaky ReLU's negative branch (mag * slope there: the bf16 module has no
    leaky kernel with a tight ruler to keep).  -> (y64, mag)."""
    if (act & 15) != 2:
        y, mag, _ = bp.epilogue(acc, mac, scale, shift, resid, act, slope)
        return y, mag
    after = bool(act & 16)
    z, m, _ = bp.epilogue(acc, mac, scale, shift, None if after else resid, 0)
    neg = z < 0
    z, m = torch.where(neg, z * slope, z), torch.where(neg, m * slope, m)
    if resid is not None and after:
        z, m = z + f64(resid), m + f64(resid).abs()
    return z, m


def chain_outputs(y64, mag, K, budget=DIRECT_BUDGET, seed=0):
    """The flat indices of the outputs whose chain c_bar_direct sums: ALL of them while n_out * K <= budget products; else budget / K
    of them, one half at random and one half the outputs with the largest |y64| / mag — the sums that cancel least, whose partial
    sums, and with them the roundings of the chain, are largest against the ruler.  (A criterion of the float64 reference alone.)"""
    y, m = np.asarray(f64(y64)).reshape(-1), np.asarray(f64(mag)).reshape(-1)
    n = max(2, budget // K)
    if y.size <= n:
        return np.arange(y.size, dtype=np.int64)
    top = np.argpartition(-(np.abs(y) / m), n // 2)[:n // 2]
    rnd = np.random.RandomState(seed).choice(y.size, n // 2, replace=False)
    return np.unique(np.concatenate([top, rnd])).astype(np.int64)


def c_bar_direct(groups, y64, mag, scale=None, shift=None, resid=None, act=0, slope=0.01, what="", budget=DIRECT_BUDGET, idx=None):
    """-> (c_bar, cap) of a direct case: the sequential fp32 chain of bf16_parity.c_bar_of on products rounded to fp32, over the outputs
    chain_outputs names, asserted under DIRECT_CAP(K).  idx: the flat outputs to sum in place of chain_outputs' choice
    (tests/update_parity.py: every output whose magnitude is not zero — an empty sum has no unit to measure an error in)."""
    K = sum(g[1] for g in groups)
    cap = DIRECT_CAP(K)
    idx = chain_outputs(y64, mag, K, budget) if idx is None else idx
    return bp.c_bar_of(groups, y64, mag, scale, shift, resid, act, slope, what=what, cap=cap, idx=idx), cap


def check32(got, y64, mag, c_bar, cap, what=""):
    """Every element of an fp32 result against the bound; prints `excess <= c_bar <= cap` in bf16_parity.line's form."""
    assert 0 < c_bar <= cap, "%s: c_bar %.3g outside (0, cap %d]" % (what, c_bar, cap)
    assert tuple(got.shape) == tuple(y64.shape), "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(y64.shape))
    return bp.check(got, y64, mag, c_bar, None, out_f32=True, what="%s [cap %d]" % (what, cap))


def trunc_mantissa(t, bits=10):
    """fp32 -> the value with its mantissa cut to `bits` explicit bits (xf32 / tf32-style operand; for mutants)."""
    a = np.ascontiguousarray(t.detach().cpu().float().numpy())
    mask = np.uint32((0xFFFFFFFF << (23 - bits)) & 0xFFFFFFFF)
    return torch.from_numpy((a.view(np.uint32) & mask).view(np.float32).copy())


# ----------------------------------------------------------------------------- Cook-Toom matrices over the rationals
def _inv(Mx):
    """Inverse of a square matrix of Fractions (Gauss-Jordan)."""
    n = len(Mx)
    a = [list(map(Fraction, r)) + [Fraction(int(i == j)) for j in range(n)] for i, r in enumerate(Mx)]
    for c in range(n):
        p = next(r for r in range(c, n) if a[r][c] != 0)
        a[c], a[p] = a[p], a[c]
        a[c] = [v / a[c][c] for v in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                a[r] = [v - a[r][c] * w for v, w in zip(a[r], a[c])]
    return [r[n:] for r in a]


def cook_toom(m):
    """F(m, 3) on POINTS[m] + infinity -> (AT [m][n], G [n][3], BT [n][n]) as lists of Fractions, n = m + 2, with
    y = AT [(G g) (.) (BT d)] = correlation(d, g).  Transposition of Toom-Cook polynomial multiplication: the product of a degree-2 and
    a degree-(m-1) polynomial has n coefficients s = C^-1 [(E3 g) (.) (Em h)] (E_k: evaluation of a k-coefficient polynomial at the points,
    the row of infinity picking the leading coefficient; C = E_n), and correlation is the transpose of that map in h."""
    n = m + 2
    pts = [Fraction(p) for p in POINTS[m]]
    assert len(pts) == n - 1 and len(set(pts)) == n - 1

    def ev(k):
        return [[p ** e for e in range(k)] for p in pts] + [[Fraction(int(e == k - 1)) for e in range(k)]]
    Ci = _inv(ev(n))
    Nrm = [Fraction(1)] * n
    for i, p in enumerate(pts):
        for j, q in enumerate(pts):
            if i != j:
                Nrm[i] *= p - q
    BT = [[Ci[c][r] * Nrm[r] for c in range(n)] for r in range(n)]          # (C^-1)^T, row r scaled by N_r
    G = [[v / Nrm[r] for v in row] for r, row in enumerate(ev(3))]
    Em = ev(m)
    AT = [[Em[r][c] for r in range(n)] for c in range(m)]
    return AT, G, BT


def fmat(Mx):
    return np.array([[float(v) for v in r] for r in Mx], dtype=np.float64)


def correlation_identity_holds(m, seed=0):
    """A^T [(G g G^T) (.) (B^T d B)] A == correlation(d, g), exactly, for integer d [n][n] and g [3][3] (object arrays of Fractions)."""
    AT, G, BT = (np.array(Mx, dtype=object) for Mx in cook_toom(m))
    n = m + 2
    r = np.random.RandomState(seed)
    d = np.array([[Fraction(int(v)) for v in row] for row in r.randint(-9, 10, (n, n))], dtype=object)
    g = np.array([[Fraction(int(v)) for v in row] for row in r.randint(-9, 10, (3, 3))], dtype=object)
    Y = AT.dot((G.dot(g).dot(G.T)) * (BT.dot(d).dot(BT.T))).dot(AT.T)
    want = [[sum(d[i + a][j + b] * g[a][b] for a in range(3) for b in range(3)) for j in range(m)] for i in range(m)]
    return all(Y[i][j] == want[i][j] for i in range(m) for j in range(m))


# ----------------------------------------------------------------------------- the host's U, un-permuted to [plane][N][Cin]
def u_from_frag(flat, m, N, Cin):
    """Inverse of encoder._winograd_u_frag: [N/32][Cin/16][P][2 nb][4 kk][16 co][4 e] -> [P][N][Cin]."""
    P = (m + 2) ** 2
    t = flat.reshape(N // 32, Cin // 16, P, 2, 4, 16, 4)                      # nt c p nb kk co e
    return t.permute(2, 0, 3, 5, 1, 4, 6).contiguous().reshape(P, N, Cin)     # p nt nb co c kk e


def u_from_c64(u8):
    """Inverse of encoder._winograd_u_c64 (cin_pairs=True): [8 chunks][16 planes][64 positions][8] -> [16][64][64]; position 16 b + n
    is output channel 4 n + b, (chunk c, index k) is input channel 16 (c // 2) + 4 (k // 2) + 2 (c % 2) + k % 2."""
    t = u8.permute(1, 2, 0, 3).reshape(16, 64, 64)                            # plane, position, 8 c + k
    pos = torch.arange(64)
    c, k = pos // 8, pos % 8
    out = torch.empty_like(t)
    tmp = torch.empty_like(t)
    tmp[:, :, 16 * (c // 2) + 4 * (k // 2) + 2 * (c % 2) + (k % 2)] = t
    out[:, 4 * (pos % 16) + pos // 16, :] = tmp
    return out


def row_scale(U_planes, w, m):
    """The diagonal D (list of n Fractions, up to a common sign) with U_stored[(i, j)] = D_i D_j (G g G^T)[i][j] for this module's
    G: fitted over row 0 of the planes, snapped to a small rational, asserted on every plane to one fp32 rounding."""
    n = m + 2
    G = torch.from_numpy(fmat(cook_toom(m)[1]))
    U0 = torch.einsum("ik,ockl,jl->ijoc", G, f64(w), G)
    Us = f64(U_planes).reshape(n, n, *U0.shape[2:])
    dot = lambda a, b: float((a * b).sum())
    d0 = np.sqrt(dot(Us[0, 0], U0[0, 0]) / dot(U0[0, 0], U0[0, 0]))
    est = [d0] + [dot(Us[0, j], U0[0, j]) / dot(U0[0, j], U0[0, j]) / d0 for j in range(1, n)]
    D = [Fraction(e).limit_denominator(4096) for e in est]
    assert all(d != 0 and abs(float(d) - e) <= 1e-5 * abs(e) for d, e in zip(D, est)), "row scales %s are no small rationals" % est
    Df = torch.tensor([float(d) for d in D], dtype=torch.float64)
    want = U0 * Df.view(n, 1, 1, 1) * Df.view(1, n, 1, 1)
    assert bool(((Us - want).abs() <= 2.0 ** -23 * want.abs() + 1e-300).all()), "stored U is not D (G g G^T) D for the points of m = %d" % m
    return D


# ----------------------------------------------------------------------------- the Winograd ruler and the fp32 emulation
def _tiles(x, m):
    """x [F][H][W][C] -> zero-padded patches [F][TH][TW][n][n][C] (pad 1 on top / left, to the tile grid + 1 below / right)."""
    Fn, H, W, C = x.shape
    n = m + 2
    TH, TW = -(-H // m), -(-W // m)
    xp = torch.zeros(Fn, TH * m + 2, TW * m + 2, C, dtype=x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    return xp.unfold(1, n, m).unfold(2, n, m).permute(0, 1, 2, 4, 5, 3)      # f th tw i j c


def wino_mag(x, U_planes, m, D):
    """sum-of-absolute-values of the Winograd form, [F][H][W][N] float64: |A^T| (sum_c |D^-1 U D^-1| (.) (|B^T| |d| |B|)) |A|."""
    AT, _, BT = cook_toom(m)
    n = m + 2
    Fn, H, W, C = x.shape
    Ba, Aa = torch.from_numpy(np.abs(fmat(BT))), torch.from_numpy(np.abs(fmat(AT)))
    Di = torch.tensor([abs(1.0 / float(d)) for d in D], dtype=torch.float64)
    Ua = f64(U_planes).abs().reshape(n, n, -1, C) * Di.view(n, 1, 1, 1) * Di.view(1, n, 1, 1)
    d = _tiles(f64(x).abs(), m)
    TH, TW = d.shape[1], d.shape[2]
    Va = torch.einsum("ik,ftwklc,jl->ijftwc", Ba, d, Ba).reshape(n * n, -1, C)
    Ma = torch.bmm(Va, Ua.reshape(n * n, -1, C).transpose(1, 2)).reshape(n, n, Fn, TH, TW, -1)
    out = torch.einsum("ik,klftwo,jl->ftiwjo", Aa, Ma, Aa).reshape(Fn, TH * m, TW * m, -1)
    return out[:, :H, :W].contiguous()


def _seq(coef, v, axis):
    """sum_k coef[:, k] v[k along axis], strictly sequential in fp32 (zero coefficients skipped).  -> axis replaced by len(coef)."""
    v = np.moveaxis(v, axis, 0)
    out = []
    for row in coef:
        acc = None
        for k, ck in enumerate(row):
            if ck == 0:
                continue
            t = v[k] if ck == 1 else np.float32(ck) * v[k]
            acc = t if acc is None else acc + t
        out.append(acc if acc is not None else np.zeros_like(v[0]))
    r = np.stack(out).astype(np.float32, copy=False)
    return np.moveaxis(r, 0, axis)


def _two_pass(coef, v, rows_first):
    """coef v coef^T over axes (1, 2) of v [S][n][n][...], one axis after the other."""
    a, b = (1, 2) if rows_first else (2, 1)
    return _seq(coef, _seq(coef, v, a), b)


def _chain(pr, chunk):
    """fp32 sum over the last axis: strictly sequential (chunk 1), or sequential partial sums of `chunk` terms added to a running sum."""
    if chunk > 1:
        C = pr.shape[-1]
        pad = -C % chunk
        if pad:
            pr = np.concatenate([pr, np.zeros(pr.shape[:-1] + (pad,), np.float32)], axis=-1)
        pr = np.cumsum(pr.reshape(pr.shape[:-1] + (-1, chunk)), axis=-1, dtype=np.float32)[..., -1]
    return np.cumsum(pr, axis=-1, dtype=np.float32)[..., -1]


def wino_emulate(x, U_planes, m, D, tiles, rows_first=True, chunk=1, quant=None):
    """The Winograd form in fp32 numpy on the tiles `tiles` ([S][3] = f, th, tw): V = B' d B'^T (B^T' = D^-1 B^T), M = sum_c V U with the
    stored U, A^T M A.  -> [S][m][m][N] fp32, before the epilogue.  quant (for mutants): applied to V and U in front of the products."""
    AT, _, BT = cook_toom(m)
    n = m + 2
    BTs = np.array([[np.float32(float(v / D[r])) for v in row] for r, row in enumerate(BT)], dtype=np.float32)
    ATs = fmat(AT).astype(np.float32)
    Un = U_planes.detach().cpu().float().numpy().reshape(n, n, -1, x.shape[-1])
    if quant is not None:
        Un = quant(torch.from_numpy(Un)).numpy()
    pat = _tiles(x.detach().cpu().float(), m)
    out = []
    step = max(1, (1 << 24) // (n * n * Un.shape[2] * Un.shape[3]))           # <= 64 MB of products at a time
    for s in range(0, len(tiles), step):
        t = tiles[s:s + step]
        d = pat[t[:, 0], t[:, 1], t[:, 2]].numpy()                            # [S][n][n][C]
        V = _two_pass(BTs, d, rows_first)
        if quant is not None:
            V = quant(torch.from_numpy(V)).numpy()
        Mx = _chain(V[:, :, :, None, :] * Un[None], chunk)                    # [S][n][n][N]
        out.append(_two_pass(ATs, Mx, rows_first))
    return np.concatenate(out)


def epilogue_np(v, scale, shift, resid, act):
    """The fp32 epilogue on [..][N] numpy arrays (resid already gathered to v's shape, or None)."""
    col = lambda t: t.detach().cpu().float().numpy()
    if scale is not None:
        v = v * col(scale)
    if shift is not None:
        v = v + col(shift)
    if resid is not None and not (act & 16):
        v = v + resid
    if (act & 15) == 1:
        v = np.maximum(v, np.float32(0))
    if resid is not None and (act & 16):
        v = v + resid
    assert v.dtype == np.float32
    return v


def _scatter(o, tiles, m, shape):
    """[S][m][m][N] tile outputs -> ([F][H][W][N] array with the tiles' pixels filled, mask of the filled pixels)."""
    Fn, H, W, N = shape
    TH, TW = -(-H // m), -(-W // m)
    full = np.zeros((Fn, TH * m, TW * m, N), o.dtype)
    mask = np.zeros((Fn, TH * m, TW * m), bool)
    for s, (f, th, tw) in enumerate(tiles):
        full[f, th * m:th * m + m, tw * m:tw * m + m] = o[s]
        mask[f, th * m:th * m + m, tw * m:tw * m + m] = True
    return full[:, :H, :W], mask[:, :H, :W]


def sample_tiles(Fn, H, W, m, n_max, seed=0):
    """All tiles when there are at most n_max, else the corner tiles of the first and the last frame plus a random sample."""
    TH, TW = -(-H // m), -(-W // m)
    grid = np.stack(np.meshgrid(np.arange(Fn), np.arange(TH), np.arange(TW), indexing="ij"), -1).reshape(-1, 3)
    if len(grid) <= n_max:
        return grid
    keep = {(f, a, b) for f in (0, Fn - 1) for a in (0, TH - 1) for b in (0, TW - 1)}
    pick = np.random.RandomState(seed).permutation(len(grid))
    for i in pick:
        if len(keep) >= n_max:
            break
        keep.add(tuple(int(v) for v in grid[i]))
    return np.array(sorted(keep), dtype=np.int64)


def wino_case(x, w, U_planes, m, scale=None, shift=None, resid=None, act=0, n_tiles=48, what="", seed=0):
    """Reference, ruler and bar of one Winograd case.  -> dict(y, mag, c_bar, cap, emu = the emulation's own worst error in units (c_bar / 2),
    ratio = median and max of mag_w / mag_direct over the conv sums, D, tiles)."""
    Fn, H, W, Cin = x.shape
    N = w.shape[0]
    D = row_scale(U_planes, w, m)
    acc, mac_d = conv_acc(x, w, 1, 1)
    mac_w = wino_mag(x, U_planes, m, D)
    y, mag, _ = epilogue(acc, mac_w, scale, shift, resid, act)
    per_tile = (m + 2) ** 2 * N * Cin
    tiles = sample_tiles(Fn, H, W, m, max(8, min(n_tiles, (1 << 25) // per_tile)), seed)
    yn, mn = y.numpy(), mag.numpy()
    rn = None if resid is None else resid.detach().cpu().float().numpy()
    worst = 0.0
    for rows_first, chunk in ORDERS:
        o, mask = _scatter(wino_emulate(x, U_planes, m, D, tiles, rows_first, chunk), tiles, m, (Fn, H, W, N))
        v = epilogue_np(o, scale, shift, rn, act)
        worst = max(worst, float((np.abs(v.astype(np.float64) - yn) / (U * mn))[mask].max()))
    c_bar, cap = FACTOR * worst, WINO_CAP(Cin, m)
    assert 0 < c_bar <= cap, "%s: c_bar %.3g outside (0, cap = %d]: the helper is wrong" % (what, c_bar, cap)
    ratio = (mac_w / mac_d.clamp_min(1e-300)).reshape(-1)
    return dict(y=y, mag=mag, c_bar=c_bar, cap=cap, emu=worst, ratio=(float(ratio.median()), float(ratio.max())), D=D, tiles=tiles)


def wino_full(x, U_planes, m, D, rows_first=True, chunk=1, quant=None):
    """The emulation on ALL tiles, before the epilogue: [F][H][W][N] fp32 array (for the CPU tests; small cases)."""
    Fn, H, W, _ = x.shape
    tiles = sample_tiles(Fn, H, W, m, 1 << 30)
    o, mask = _scatter(wino_emulate(x, U_planes, m, D, tiles, rows_first, chunk, quant), tiles, m, (Fn, H, W, U_planes.shape[1]))
    assert mask.all()
    return np.ascontiguousarray(o)


def old_metric(got, ref):
    """max|got - ref| / max|ref|: the metric of the fp32 tests in tests/test_kernels_gpu.py (bar 2e-5; 1e-4 for F(6x6))."""
    return bp.old_metric(got, ref)


def log_scales(r, N):
    """Per-channel scales log-uniform over [1e-2, 1e1] with random sign (folded BN scales span decades), fp32 tensor."""
    return torch.from_numpy((10.0 ** r.uniform(-2, 1, N) * r.choice([-1.0, 1.0], N)).astype(np.float32))
