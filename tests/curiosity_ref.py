"""Float64 statement of the curiosity module (cadre_amd/curiosity.py, csrc/curiosity.hip) with running first-order error bounds.

Every device quantity is stated as a (value, error) pair in the manner of tests/loss_parity.py: `value` is the exact-arithmetic
float64 result, `error` an a-priori bound on what the fp32 kernels may deviate by.  U = 2^-24 is fp32's half-ulp.  A dot product of
depth k contributes (k + 2) U sum |a_i b_i| whatever its summation order; every elementwise statement adds its own half-ulp; input
errors propagate through |W|.  At a ReLU whose float64 pre-activation lies within its own bound of zero either branch is accepted
(the element's error becomes max(error, |pre|)) and in the backward pass such a unit's whole contribution joins the bound.
Nothing here is taken from the device."""
import numpy as np

U = 2.0 ** -24
M64 = (1 << 64) - 1
RND_N, RND_BETA, RND_EXT, RND_RHO_N, RND_RHO_MEAN, RND_RHO_M2, RND_SIGMA, RND_KEY, RND_CTR, RND_HEAD = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16


def tower_offsets(D, H, E):
    o = [0, D * H, D * H + H, D * H + H + H * H, D * H + 2 * H + H * H, D * H + 2 * H + H * H + H * E]
    return o, o[5] + E


def unpack(p, D, H, E):
    """(W1 [D][H], b1, W2 [H][H], b2, W3 [H][E], b3) of a flat tower buffer, float64."""
    p = np.asarray(p, np.float64)
    o, P = tower_offsets(D, H, E)
    assert p.size == P
    return (p[o[0]:o[1]].reshape(D, H), p[o[1]:o[2]], p[o[2]:o[3]].reshape(H, H), p[o[3]:o[4]], p[o[4]:o[5]].reshape(H, E), p[o[5]:])


def pack(parts):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in parts])


# ----------------------------------------------------------------------------- the mask generator
def mask_bits(key, ctr):
    z = (key * 0x9E3779B97F4A7C15 + ctr) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return z >> 40


def mask(key, ctr, rows, update_proportion):
    """m [rows] (bool): the top 24 bits of splitmix64(key * golden + ctr + i) below update_proportion * 2^24."""
    thresh = int(float(update_proportion) * float(1 << 24))
    return np.array([mask_bits(int(key), int(ctr) + i) < thresh for i in range(rows)], dtype=bool)


# ----------------------------------------------------------------------------- running statistics
def chan_merge(n, mu, M2, X):
    """Chan's merge of the rows of X [R][...] into (n, mu, M2); the batch's mean and squared deviations in one numpy pass."""
    X = np.asarray(X, np.float64)
    nb = float(X.shape[0])
    mean = X.mean(0)
    q = ((X - mean) ** 2).sum(0)
    tot = n + nb
    delta = mean - mu
    return tot, mu + delta * nb / tot, M2 + q + delta * delta * n * nb / tot


def rho_scan(err, carry, gamma):
    """rho [N][T] and the carries behind it: rho <- gamma rho + err[w][t], forward in time, no reset."""
    err = np.asarray(err, np.float64)
    rho = np.zeros_like(err)
    c = np.array(carry, np.float64)
    for t in range(err.shape[1]):
        c = gamma * c + err[:, t]
        rho[:, t] = c
    return rho, c


def reward(err, carry, stats, gamma, eps, beta, ext, rewards):
    """err [N][T] (the device's float32 values, taken as exact), stats = (n, mean, M2) of rho -> (new stats, carries, sigma, (mixed,
    error)) with rewards [2N][T] and mixed_k = ext r_k + beta err[k // 2] / (float)sigma."""
    err = np.asarray(err, np.float64)
    rho, c = rho_scan(err, carry, gamma)
    n, mean, M2 = chan_merge(stats[0], stats[1], stats[2], rho.reshape(-1))
    sigma = np.sqrt(M2 / n + eps)
    return (n, mean, M2), c, sigma, mixed(err, sigma, beta, ext, rewards)


def mixed(err, sigma, beta, ext, rewards):
    err, r = np.asarray(err, np.float64), np.asarray(rewards, np.float64)
    ri = np.repeat(err / sigma, 2, axis=0)
    e_ri = 2 * U * np.abs(ri)                            # (float)sigma, the division
    a, b = ext * r, beta * ri
    v = a + b
    return v, 2 * U * np.abs(a) + abs(beta) * e_ri + 2 * U * np.abs(b) + U * np.abs(v)


# ----------------------------------------------------------------------------- forward
def normalise(x, n, mu, M2, eps, clip):
    x = np.asarray(x, np.float64)
    sd = np.sqrt((M2 / n if n > 0 else np.ones_like(M2)) + eps)
    num = x - mu
    e_num = U * np.abs(mu) + U * np.abs(num)
    q = num / sd
    e_q = e_num / sd + 2 * U * np.abs(q)
    return np.clip(q, -clip, clip), e_q


def dense(A, eA, W, b):
    K = A.shape[1]
    pre = A @ W + b
    e = eA @ np.abs(W) + (K + 2) * U * (np.abs(A) @ np.abs(W)) + U * np.abs(pre)
    return pre, e


def relu(pre, e):
    """(value, error, ambiguous)."""
    amb = np.abs(pre) <= e
    h = np.maximum(pre, 0.0)
    eh = np.where(amb, np.maximum(e, np.abs(pre)), np.where(pre > 0, e, 0.0))
    return h, eh, amb


def tower(xh, e_xh, p, D, H, E):
    W1, b1, W2, b2, W3, b3 = unpack(p, D, H, E)
    p1, e1 = dense(xh, e_xh, W1, b1)
    h1, eh1, a1 = relu(p1, e1)
    p2, e2 = dense(h1, eh1, W2, b2)
    h2, eh2, a2 = relu(p2, e2)
    o, eo = dense(h2, eh2, W3, b3)
    return dict(h1=(h1, eh1), h2=(h2, eh2), o=(o, eo), amb1=a1, amb2=a2, pre1=p1, pre2=p2)


def forward(x, n, mu, M2, target, predictor, H, E, clip=5.0, eps=1e-8):
    """x [R][D] float32 rows -> dict of (value, error) pairs: xh, h1, h2 (the predictor's), diff, err; `f`, `g`: the towers."""
    D = x.shape[1]
    xh, e_xh = normalise(x, n, mu, M2, eps, clip)
    f, g = tower(xh, e_xh, target, D, H, E), tower(xh, e_xh, predictor, D, H, E)
    d = g["o"][0] - f["o"][0]
    e_d = g["o"][1] + f["o"][1] + U * np.abs(d)
    s = (d * d).sum(1)
    e_s = (2 * np.abs(d) * e_d).sum(1) + (E + 2) * U * s
    err = s / E
    return dict(xh=(xh, e_xh), h1=g["h1"], h2=g["h2"], diff=(d, e_d), err=(err, e_s / E + U * err), f=f, g=g)


def ambiguity(fw):
    """The share of units whose ReLU branch the bound cannot decide, per tower and layer."""
    return {(t, k): float(fw[t]["amb%d" % k].mean()) for t in ("f", "g") for k in (1, 2)}


# ----------------------------------------------------------------------------- backward
def backward(fw, predictor, m, H, E):
    """The gradient of L = sum m err / max(sum m, 1) in the predictor's flat layout as a (value, error) pair, and dO."""
    xh, e_xh = fw["xh"]
    h1, eh1 = fw["h1"]
    h2, eh2 = fw["h2"]
    d, e_d = fw["diff"]
    g = fw["g"]
    R, D = xh.shape
    W1, _b1, W2, _b2, W3, _b3 = unpack(predictor, D, H, E)
    m = np.asarray(m, np.float64).reshape(R, 1)
    den = E * max(m.sum(), 1.0)
    dO = 2.0 * m * d / den
    e_dO = 2.0 * m * e_d / den + U * np.abs(dO)

    def wgrad(A, eA, G, eG):
        v = A.T @ G
        e = (R + 2) * U * (np.abs(A).T @ np.abs(G)) + eA.T @ np.abs(G) + np.abs(A).T @ eG
        return v, e, G.sum(0), (R + 2) * U * np.abs(G).sum(0) + eG.sum(0)

    def back(G, eG, W, pre, amb):
        K = G.shape[1]
        v = G @ W.T
        e = (K + 2) * U * (np.abs(G) @ np.abs(W.T)) + eG @ np.abs(W.T)
        on = pre > 0
        return np.where(on, v, 0.0), np.where(amb, e + np.abs(v), np.where(on, e, 0.0))

    dW3, e_dW3, db3, e_db3 = wgrad(h2, eh2, dO, e_dO)
    dH2, e_dH2 = back(dO, e_dO, W3, g["pre2"], g["amb2"])
    dW2, e_dW2, db2, e_db2 = wgrad(h1, eh1, dH2, e_dH2)
    dH1, e_dH1 = back(dH2, e_dH2, W2, g["pre1"], g["amb1"])
    dW1, e_dW1, db1, e_db1 = wgrad(xh, e_xh, dH1, e_dH1)
    return (pack([dW1, db1, dW2, db2, dW3, db3]), pack([e_dW1, e_db1, e_dW2, e_db2, e_dW3, e_db3])), (dO, e_dO)


def loss(fw, m):
    m = np.asarray(m, np.float64)
    return float((m * fw["err"][0]).sum() / max(m.sum(), 1.0))


# ----------------------------------------------------------------------------- a float64 training run (the distillation test)
def adam_run(x, n, mu, M2, target, predictor, H, E, steps, lr, clip=5.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """`steps` full-batch predictor steps (mask all ones) with torch's Adam rule in float64; returns the predictor."""
    p = np.asarray(predictor, np.float64).copy()
    mo, vo = np.zeros_like(p), np.zeros_like(p)
    ones = np.ones(x.shape[0])
    for t in range(1, steps + 1):
        (g, _e), _ = backward(forward(x, n, mu, M2, target, p, H, E, clip), p, ones, H, E)
        mo = beta1 * mo + (1 - beta1) * g
        vo = beta2 * vo + (1 - beta2) * g * g
        p = p - lr / (1 - beta1 ** t) * mo / (np.sqrt(vo) / np.sqrt(1 - beta2 ** t) + eps)
    return p


def within(got, pair):
    """(worst ratio |got - value| / error, count outside) of a device array against a (value, error) pair.  The bound is taken as it
    is (plus the smallest subnormal, for elements whose bound is an exact zero); a NaN or an infinity counts as outside."""
    v, e = pair
    got = np.asarray(got, np.float64).reshape(v.shape)
    dev = np.abs(got - v)
    lim = e + 2.0 ** -149
    ok = dev <= lim                                       # (False for NaN)
    ratio = float(np.nanmax(dev / lim)) if dev.size else 0.0
    return (ratio if bool(np.isfinite(got).all()) else float("inf")), int((~ok).sum())
