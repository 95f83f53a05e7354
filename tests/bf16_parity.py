"""Element-wise float64 parity bound for the bf16 (config C3) kernels — the bound, stated once ("bf16 parity").

The kernels read exact bf16 operands, form products that are exact in fp32, accumulate in fp32 and round ONCE to bf16.
A float64 reference on the operands as stored therefore pins every output element to

    |got - y64|  <=  1/2 ulp_bf16(y64)  +  c_bar * unit,        unit = 2^-24 * mag,

`mag` being the reference expression with every operand replaced by its absolute value (|scale| sum|a||b| + |shift| + |resid|).
`c_bar` is never taken from a kernel: `c_bar_of` accumulates a sample of the same sums strictly sequentially in fp32 on the CPU
(np.cumsum over the products: the least favourable order a kernel here can use — MFMA chunks only shorten the chains), runs
the fp32 epilogue on them, takes the worst error over float64 in units and doubles it (margin for the maximum over a sample
being a random quantity and for the few fp32 epilogue operations).  It asserts c_bar <= K + 4, the worst case of ANY order.

Plain helper module (no GPU, no fixtures): tests/test_bf16_parity_cpu.py shows that the bound has teeth, tests/test_bf16_parity_gpu.py
applies it to the kernels.  Tensors are torch CPU tensors; activations are NHWC, conv weights OIHW.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # one unit = U * mag
SHARE_CAP = 1e-3          # share of elements allowed to differ from RNE_bf16(y64) (each by one bf16 step)
BIAS_SE = 6.0             # rounding bias bar: six standard errors of a uniform +-1/2 rounding error
SD_UNIFORM = 0.2887       # 1 / sqrt(12)
BIAS_MIN_UNITS = 64.0     # the bias is taken where ulp_bf16(y64) >= 64 units (rounding dominates the accumulation error)
MIN_EXP = -126            # smallest normal exponent of bf16 (and fp32)


# ----------------------------------------------------------------------------- number formats
def f64(t):
    """A stored operand (bf16 / fp32 tensor or array) widened to float64, exactly."""
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().to(torch.float64)
    return torch.from_numpy(np.asarray(t, dtype=np.float64))


def ulp_bf16(y):
    """2^(floor(log2|y|) - 7), the exponent floored at the smallest normal one (float64 ndarray in, ndarray out)."""
    y = np.asarray(y, dtype=np.float64)
    _, e = np.frexp(y)                                   # |y| = m 2^e, m in [0.5, 1): floor(log2|y|) = e - 1
    e = np.where(y == 0, MIN_EXP, e - 1)
    return np.ldexp(1.0, np.maximum(e, MIN_EXP) - 7)


def rne_bf16(y):
    """float64 -> nearest bf16 value (ties to even), rounded from float64 DIRECTLY, not through fp32.  Returned as float64."""
    y = np.asarray(y, dtype=np.float64)
    u = ulp_bf16(y)
    return np.rint(y / u) * u                            # (y / u is exact: u is a power of two; rint rounds ties to even)


def trunc_bf16(v32):
    """fp32 -> bf16 by dropping the low 16 bits (the WRONG conversion; for mutants)."""
    a = np.ascontiguousarray(v32.detach().cpu().numpy() if isinstance(v32, torch.Tensor) else v32, dtype=np.float32)
    return torch.from_numpy((a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)).to(torch.bfloat16)


def _bf16_order(v64):
    """bf16 values (as float64) -> integers that count bf16 steps along the real line (-0 and +0 coincide)."""
    b = torch.from_numpy(np.asarray(v64, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFF))


# ----------------------------------------------------------------------------- float64 references (value, magnitude)
def _nchw(x):
    return f64(x).permute(0, 3, 1, 2)


def conv_acc(x, w, stride=1, pad=1):
    """x NHWC, w OIHW (any KH x KW, any stride / padding) -> (sum, sum of |a||b|), both float64 NHWC."""
    xd, wd = _nchw(x), f64(w)
    acc = F.conv2d(xd, wd, None, stride, pad)
    mac = F.conv2d(xd.abs(), wd.abs(), None, stride, pad)
    return acc.permute(0, 2, 3, 1).contiguous(), mac.permute(0, 2, 3, 1).contiguous()


def shortcut_acc(x2, wd):
    """The 1x1 / stride-2 shortcut of a down-sampling block: x2 NHWC [F][2H][2W][Cd], wd [O][Cd][1][1]."""
    return conv_acc(x2, wd, 2, 0)


def dense_acc(A, B, chunk=256):
    """A [M][K], B [N][K] -> (A B^T, |A| |B|^T) in float64 (B taken `chunk` rows at a time: K = 41472 stays small in memory)."""
    Ad = f64(A)
    Aa = Ad.abs()
    acc, mac = [], []
    for s in range(0, B.shape[0], chunk):
        Bd = f64(B[s:s + chunk])
        acc.append(Ad @ Bd.t())
        mac.append(Aa @ Bd.abs().t())
    return torch.cat(acc, 1), torch.cat(mac, 1)


def epilogue(acc, mac, scale=None, shift=None, resid=None, act=0, slope=0.01):
    """act(scale acc + shift (+ resid)) with the residual after the activation when act & 16; act & 15: 0 none, 1 ReLU,
    2 leaky ReLU(slope).  scale / shift broadcast over the last axis.  -> (y64, mag, clamped): clamped marks the elements a
    ReLU set to zero (their rounding error is not uniform: the bias statistic leaves them out)."""
    z, m = acc, mac
    if scale is not None:
        z, m = z * f64(scale), m * f64(scale).abs()
    if shift is not None:
        z, m = z + f64(shift), m + f64(shift).abs()
    after = bool(act & 16)
    if resid is not None and not after:
        z, m = z + f64(resid), m + f64(resid).abs()
    clamped = torch.zeros_like(z, dtype=torch.bool)
    if (act & 15) == 1:
        clamped = z <= 0
        z = torch.relu(z)
    elif (act & 15) == 2:
        z = torch.where(z < 0, z * slope, z)
    if resid is not None and after:
        z, m = z + f64(resid), m + f64(resid).abs()
    return z, m, clamped


def pool_ref(y, mag, clamped):
    """max_pool2d(3, 2, 1) behind a reference (NHWC): rounding is monotone, so the pooled element is the rounded maximum and
    still owes half an ulp; mag / clamped are those of the element the maximum picked."""
    yn = y.permute(0, 3, 1, 2)
    p, idx = F.max_pool2d(yn, 3, 2, 1, return_indices=True)
    Fn, C = yn.shape[:2]
    pm = mag.permute(0, 3, 1, 2).reshape(Fn, C, -1).gather(2, idx.reshape(Fn, C, -1)).reshape(p.shape)
    pc = clamped.permute(0, 3, 1, 2).reshape(Fn, C, -1).gather(2, idx.reshape(Fn, C, -1)).reshape(p.shape)
    return p.permute(0, 2, 3, 1).contiguous(), pm.permute(0, 2, 3, 1).contiguous(), pc.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------- c_bar: sequential fp32 accumulation on the CPU
def conv_products(x, w, stride=1, pad=1):
    """-> products(flat output indices) = [S][KH*KW*Cin] fp32, the im2col row of each sampled output element times its weight
    row (bf16 x bf16 is exact in fp32), and K.  Output layout [F][Ho][Wo][O] flat."""
    xf = x.detach().cpu().float()
    wf = w.detach().cpu().float().permute(0, 2, 3, 1).contiguous()            # [O][KH][KW][Cin]
    Fn, H, W, Cin = xf.shape
    O, KH, KW, _ = wf.shape
    xp = F.pad(xf, (0, 0, pad, pad, pad, pad)).numpy()
    wn = wf.numpy()
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    kh, kw = np.meshgrid(np.arange(KH), np.arange(KW), indexing="ij")

    def products(idx):
        n = idx % O
        wo = idx // O % Wo
        ho = idx // (O * Wo) % Ho
        f = idx // (O * Wo * Ho)
        patch = xp[f[:, None, None], (ho * stride)[:, None, None] + kh, (wo * stride)[:, None, None] + kw]   # [S][KH][KW][Cin]
        return (patch * wn[n]).reshape(len(idx), -1)
    return products, KH * KW * Cin, Fn * Ho * Wo * O


def dense_products(A, B):
    An, Bn = A.detach().cpu().float().numpy(), B.detach().cpu().float().numpy()
    N = Bn.shape[0]

    def products(idx):
        return An[idx // N] * Bn[idx % N]
    return products, An.shape[1], An.shape[0] * N


def c_bar_of(groups, y64, mag, scale=None, shift=None, resid=None, act=0, slope=0.01, n_sample=4096, seed=0, what="", cap=None, idx=None):
    """c_bar of one test case.  groups: [(products, K, n_out)] from conv_products / dense_products — several groups form ONE
    accumulation (the shortcut of cadre_conv3x3_s1x rides behind conv2's k-tiles).  A sample of output elements is summed strictly
    sequentially in fp32, the fp32 epilogue applied, and the worst error against y64 in units doubled.  y64 / mag: the float64
    reference of the SAME (pre-pool) outputs, flat in the products' output order.  cap: the a-priori bound c_bar is asserted under
    (default K + 4, the bf16 kernels' exact products; tests/f32_parity.py passes the one it derives for rounded fp32 products).  idx: the
    flat output indices to sum in place of the random sample (tests/f32_parity.py: every output of a small case)."""
    y = np.asarray(f64(y64)).reshape(-1)
    m = np.asarray(f64(mag)).reshape(-1)
    n_out = groups[0][2]
    assert all(g[2] == n_out for g in groups) and y.size == n_out
    K = sum(g[1] for g in groups)
    N = y64.shape[-1]
    if idx is None:
        idx = np.sort(np.random.RandomState(seed).choice(n_out, min(n_sample, n_out), replace=False)).astype(np.int64)
    step = max(1, (1 << 24) // K)                          # <= 64 MB of products at a time
    acc = np.empty(len(idx), np.float32)
    for s in range(0, len(idx), step):
        pr = np.concatenate([g[0](idx[s:s + step]).astype(np.float32) for g in groups], axis=1)
        acc[s:s + step] = np.cumsum(pr, axis=1, dtype=np.float32)[:, -1]        # strictly sequential fp32 chain over k
    col = lambda t: None if t is None else t.detach().cpu().float().numpy().reshape(-1)
    v = acc
    if scale is not None:
        v = v * col(scale)[idx % N]
    if shift is not None:
        v = v + col(shift)[idx % N]
    r = None if resid is None else col(resid)[idx]
    if r is not None and not (act & 16):
        v = v + r
    if (act & 15) == 1:
        v = np.maximum(v, np.float32(0))
    elif (act & 15) == 2:
        v = np.where(v < 0, v * np.float32(slope), v)
    if r is not None and (act & 16):
        v = v + r
    assert v.dtype == np.float32
    worst = float(np.max(np.abs(v.astype(np.float64) - y[idx]) / (U * m[idx])))
    c_bar = 2.0 * worst
    cap = K + 4 if cap is None else cap
    assert 0 < c_bar <= cap, "%s: c_bar %.3g outside (0, cap = %d]: the helper is wrong" % (what, c_bar, cap)
    return c_bar


# ----------------------------------------------------------------------------- the check
def measure(got, y64, mag, c_bar, clamped=None, out_f32=False):
    """The three quantities of the bound for a kernel result `got` (bf16 tensor, or fp32 when out_f32: no half-ulp term, no
    rounding statistics).  -> dict(excess, c_bar, share, far, bias, n_bias, bias_bar, n, worst=flat index of the worst excess)."""
    g = np.asarray(f64(got)).reshape(-1)
    y = np.asarray(f64(y64)).reshape(-1)
    m = np.asarray(f64(mag)).reshape(-1)
    assert g.shape == y.shape == m.shape and g.size > 0
    assert np.isfinite(g).all(), "non-finite output"
    unit = U * m
    assert (unit > 0).all()
    err = np.abs(g - y)
    st = dict(c_bar=float(c_bar), n=int(g.size), share=0.0, far=0, bias=0.0, n_bias=0, bias_bar=0.0)
    if out_f32:
        ex = err / unit
    else:
        u = ulp_bf16(y)
        ex = (err - 0.5 * u) / unit
        want = rne_bf16(y)
        diff = g != want
        st["share"] = float(diff.mean())
        # a mismatch is the neighbouring bf16 value wherever the accumulation slack is shorter than half a bf16 step (the spacing
        # below a power of two is ulp / 2): the fp32 value then lies across at most ONE rounding boundary from y64.  Elements next
        # to zero, whose bf16 steps are finer than the slack (a ReLU'd sum of -1e-9 against +1e-9), answer to the excess alone.
        diff_adj = diff & (c_bar * unit < 0.25 * u)
        if diff_adj.any():
            st["far"] = int((np.abs(_bf16_order(g[diff_adj]) - _bf16_order(want[diff_adj])) > 1).sum())
        sel = u >= BIAS_MIN_UNITS * unit
        if clamped is not None:
            sel &= ~np.asarray(clamped).reshape(-1)
        st["n_bias"] = int(sel.sum())
        if st["n_bias"]:
            st["bias"] = float(np.mean((g[sel] - y[sel]) / u[sel]))
            st["bias_bar"] = BIAS_SE * SD_UNIFORM / np.sqrt(st["n_bias"])
    st["worst"] = int(np.argmax(ex))
    st["excess"] = float(ex[st["worst"]])
    return st


def line(what, st):
    return ("%s: excess %.3f units (c_bar %.3f), mismatch share %.2e (%d not adjacent), bias %+.4f ulp over n=%d (bar %.4f), %d elements"
            % (what, st["excess"], st["c_bar"], st["share"], st["far"], st["bias"], st["n_bias"], st["bias_bar"], st["n"]))


def failures(st, out_f32=False, need_bias_n=0):
    """The conditions of the bound that `st` breaks (empty: accepted)."""
    bad = []
    if not st["excess"] <= st["c_bar"]:
        bad.append("excess %.3f units > c_bar %.3f (flat index %d)" % (st["excess"], st["c_bar"], st["worst"]))
    if not out_f32:
        if not st["share"] <= SHARE_CAP:
            bad.append("mismatch share %.2e > %.0e" % (st["share"], SHARE_CAP))
        if st["far"]:
            bad.append("%d mismatching elements are not an adjacent bf16 value" % st["far"])
        if st["n_bias"] < need_bias_n:
            bad.append("bias sample n=%d < %d: choose larger inputs" % (st["n_bias"], need_bias_n))
        if st["n_bias"] and not abs(st["bias"]) <= st["bias_bar"]:
            bad.append("rounding bias %+.4f ulp beyond %.4f (n=%d)" % (st["bias"], st["bias_bar"], st["n_bias"]))
    return bad


def check(got, y64, mag, c_bar, clamped=None, out_f32=False, what="", need_bias_n=0):
    """measure + print one line + assert the bound.  Returns the statistics."""
    st = measure(got, y64, mag, c_bar, clamped, out_f32)
    print(line(what, st))
    bad = failures(st, out_f32, need_bias_n)
    if bad:                                                  # where: the element of the worst excess, value against reference
        at = tuple(int(i) for i in np.unravel_index(st["worst"], tuple(y64.shape)))
        g, y = float(f64(got).reshape(-1)[st["worst"]]), float(f64(y64).reshape(-1)[st["worst"]])
        bad.append("worst element %s of %s: got %.9g, float64 %.9g, mag %.4g" % (at, tuple(y64.shape), g, y, float(f64(mag).reshape(-1)[st["worst"]])))
    assert not bad, "%s: %s" % (what, "; ".join(bad))
    return st


def old_metric(got, ref):
    """max|got - ref| / max|ref|: the metric of the existing bf16 tests (bars 5e-3 ... 1.5e-2)."""
    g, r = f64(got), f64(ref)
    return float((g - r).abs().max() / r.abs().max())
