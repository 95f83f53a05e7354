"""Float64 statement of the cost-constraint module (cadre_amd/constraint.py, csrc/constraint.hip) with running first-order error
bounds, in the manner of tests/curiosity_ref.py (whose `dense`, `relu`, `within` and U = 2^-24 it uses): every device quantity of the
cost critic is a (value, error) pair; the multiplier rule is float64; the mix is stated in numpy float32, one rounded operation per
statement, for a bit-for-bit comparison.  Nothing here is taken from the device."""
import numpy as np

from tests.curiosity_ref import U, dense, relu, within  # noqa: F401

LAG_LAMBDA, LAG_BUDGET, LAG_LR, LAG_MAX, LAG_J, LAG_SHARE, LAG_UPDATES, LAG_STRIDE = 0, 1, 2, 3, 4, 5, 6, 8
f32 = np.float32


def tower_offsets(D, H):
    o = [0, D * H, D * H + H, D * H + H + H * H, D * H + 2 * H + H * H, D * H + 3 * H + H * H]
    return o, o[5] + 1


def unpack(p, D, H):
    """(W1 [D][H], b1, W2 [H][H], b2, W3 [H][1], b3 [1]) of a flat cost tower, float64."""
    p = np.asarray(p, np.float64)
    o, P = tower_offsets(D, H)
    assert p.size == P
    return (p[o[0]:o[1]].reshape(D, H), p[o[1]:o[2]], p[o[2]:o[3]].reshape(H, H), p[o[3]:o[4]], p[o[4]:o[5]].reshape(H, 1), p[o[5]:])


def pack(parts):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in parts])


# ----------------------------------------------------------------------------- the cost critic
def forward(x, p, H):
    """x [R][D] float32 rows as stored (exact) -> dict of (value, error) pairs h1, h2, v [R]; pre-activations and ambiguity masks."""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    W1, b1, W2, b2, W3, b3 = unpack(p, D, H)
    p1, e1 = dense(x, np.zeros_like(x), W1, b1)
    h1, eh1, a1 = relu(p1, e1)
    p2, e2 = dense(h1, eh1, W2, b2)
    h2, eh2, a2 = relu(p2, e2)
    v, ev = dense(h2, eh2, W3, b3)                       # (a dot product of depth H in k order, then the bias)
    return dict(x=x, h1=(h1, eh1), h2=(h2, eh2), v=(v[:, 0], ev[:, 0]), amb1=a1, amb2=a2, pre1=p1, pre2=p2)


def ambiguity(fw):
    """The share of units whose ReLU branch the bound cannot decide, per layer."""
    return {k: float(fw["amb%d" % k].mean()) for k in (1, 2)}


def backward(fw, p, ret, H):
    """The gradient of L = 0.5 mean (v - ret)^2 in the tower's flat layout as a (value, error) pair, the loss pair and dv."""
    x = fw["x"]
    h1, eh1 = fw["h1"]
    h2, eh2 = fw["h2"]
    v, ev = fw["v"]
    R, D = x.shape
    _W1, _b1, W2, _b2, W3, _b3 = unpack(p, D, H)
    ret = np.asarray(ret, np.float64)
    d = v - ret
    e_d = ev + U * np.abs(d)
    dv = d / R
    e_dv = e_d / R + U * np.abs(dv)
    loss = 0.5 * (d * d).mean()
    e_loss = 0.5 * (2 * np.abs(d) * e_d + e_d * e_d).mean() + 2 * U * loss      # (a float64 sum of the device's d^2, one cast)

    def wgrad(A, eA, G, eG):
        val = A.T @ G
        e = (R + 2) * U * (np.abs(A).T @ np.abs(G)) + eA.T @ np.abs(G) + np.abs(A).T @ eG
        return val, e, G.sum(0), (R + 2) * U * np.abs(G).sum(0) + eG.sum(0)

    def back(G, eG, W, pre, amb):
        K = G.shape[1]
        val = G @ W.T
        e = (K + 2) * U * (np.abs(G) @ np.abs(W.T)) + eG @ np.abs(W.T)
        on = pre > 0
        return np.where(on, val, 0.0), np.where(amb, e + np.abs(val), np.where(on, e, 0.0))

    G3, eG3 = dv.reshape(R, 1), e_dv.reshape(R, 1)
    dW3, e_dW3, db3, e_db3 = wgrad(h2, eh2, G3, eG3)
    val = G3 * W3.T                                      # one product per element
    e = eG3 * np.abs(W3.T) + U * np.abs(val)
    on = fw["pre2"] > 0
    dH2, e_dH2 = np.where(on, val, 0.0), np.where(fw["amb2"], e + np.abs(val), np.where(on, e, 0.0))
    dW2, e_dW2, db2, e_db2 = wgrad(h1, eh1, dH2, e_dH2)
    dH1, e_dH1 = back(dH2, e_dH2, W2, fw["pre1"], fw["amb1"])
    dW1, e_dW1, db1, e_db1 = wgrad(x, np.zeros_like(x), dH1, e_dH1)
    return ((pack([dW1, db1, dW2, db2, dW3, db3]), pack([e_dW1, e_db1, e_dW2, e_db2, e_dW3, e_db3])), (loss, e_loss), (dv, e_dv))


def adam_run(x, p, ret, H, steps, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """`steps` full-batch critic steps with torch's Adam rule in float64; returns the tower."""
    p = np.asarray(p, np.float64).copy()
    mo, vo = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, steps + 1):
        (g, _e), _l, _d = backward(forward(x, p, H), p, ret, H)
        mo = beta1 * mo + (1 - beta1) * g
        vo = beta2 * vo + (1 - beta2) * g * g
        p = p - lr / (1 - beta1 ** t) * mo / (np.sqrt(vo) / np.sqrt(1 - beta2 ** t) + eps)
    return p


def loss(x, p, ret, H):
    return float(0.5 * ((forward(x, p, H)["v"][0] - np.asarray(ret, np.float64)) ** 2).mean())


# ----------------------------------------------------------------------------- the multiplier
def lambda_step(costs, lam, budget, lr, lam_max, train=True):
    """costs: the head's N T float32 costs -> (J, share of rows with c > 0, the new lambda), float64."""
    c = np.asarray(costs, np.float64).reshape(-1)
    J = float(c.sum() / c.size)
    share = float((c > 0).sum() / c.size)
    if train:
        lam = min(max(lam + lr * (J - budget), 0.0), lam_max)
    return J, share, lam


# ----------------------------------------------------------------------------- the mix, bit for bit
def mix(adv_r, adv_c, lam):
    """adv_r, adv_c float32 [T], lam float64 -> (advantages float32 [T], m).  (float)lam == 0: adv_r itself, no statement runs."""
    adv_r, adv_c = np.asarray(adv_r, f32), np.asarray(adv_c, f32)
    lf = f32(lam)
    T = adv_c.size
    s = np.cumsum(adv_c.astype(np.float64))[-1]          # a sequential float64 sum in row order
    m = f32(f32(s) / f32(T))
    if lf == 0:
        return adv_r, m
    c = (adv_c - m).astype(f32)
    p = (lf * c).astype(f32)
    q = (adv_r - p).astype(f32)
    return (q / f32(f32(1.0) + lf)).astype(f32), m


def case_inputs(D, N, T, H, seed):
    """Per head the rows [N (T + 1)][D] of unit normals in (storage, time) order and an orthogonal tower: what the parity tests
    use."""
    import torch
    from cadre_amd.constraint import init_cost_tower
    rng = np.random.RandomState(seed)
    x = [rng.randn(N * (T + 1), D).astype(np.float32) for _h in (0, 1)]
    gen = torch.Generator()
    gen.manual_seed(seed)
    return x, [init_cost_tower(D, H, gen).numpy() for _h in (0, 1)]
