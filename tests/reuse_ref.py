"""Reference arithmetic of sample reuse (csrc/reuse.hip): a float64 V-trace, the fp32 numpy emulation of vtrace_multi_kernel's
statements (one rounded operation per line, the normalisation's lane-strided double sums and shuffle tree included) with its
one-statement mutants, and the float64 diagnostics.  Plain helper module (no GPU, no fixtures).

What a host cannot reproduce is expf: the emulation takes the ratio as an argument (the GPU tests hand it the kernel's own
stored ratio, after checking that against float64 exp at update_parity.T_EXP ulps)."""
import numpy as np

f32, f64 = np.float32, np.float64
MUTANTS = ("rho_twice", "no_cw", "keep_one_chain", "boot_product")


def stage_rewards32(r, scale=None, clip=None):
    """The staged reward: clamp(r * scale, -clip, clip) with a scaler state, else r."""
    r = np.asarray(r, f32).copy()
    if scale is not None:
        r = (r * f32(scale)).astype(f32)
        r = np.minimum(np.maximum(r, f32(-clip)), f32(clip)).astype(f32)
    return r


def scan32(r, V, m, keep, ratio, boot_keep, gamma, gamma_tau, rho_bar, c_bar, scale=None, clip=None, mutant=None):
    """vtrace_multi_kernel's scan in float32.  r, V, m, keep: T + 1 values (keep = 1 - time_limit; None: ones); ratio: T values.
    Returns (returns [T], raw advantages a_t [T], V with the bootstrap the scan used, rho [T])."""
    assert mutant is None or mutant in MUTANTS
    T = len(ratio)
    r = stage_rewards32(r, scale, clip)
    V = np.asarray(V, f32).copy()
    m = np.asarray(m, f32)
    keep = np.ones(T + 1, f32) if keep is None else np.asarray(keep, f32)
    ratio = np.asarray(ratio, f32)
    g, gt, rb, cb = f32(gamma), f32(gamma_tau), f32(rho_bar), f32(c_bar)
    if mutant == "boot_product":
        V[T] = f32(f32(boot_keep) * V[T])
    else:
        V[T] = V[T] if f32(boot_keep) != f32(0.0) else f32(0.0)
    rho = np.minimum(rb, ratio).astype(f32)
    cw = np.minimum(cb, ratio).astype(f32)
    ret, adv = np.zeros(T, f32), np.zeros(T, f32)
    acc = f32(0.0)
    for t in range(T - 1, -1, -1):
        t1 = f32(g * V[t + 1])
        t2 = f32(t1 * m[t])
        t3 = f32(r[t] + t2)
        delta = f32(t3 - V[t])
        u1 = f32(gt * m[t])
        a2 = f32(u1 * acc)
        A = f32(delta + a2)
        if mutant != "keep_one_chain":
            A = f32(A * keep[t])
        rd = f32(rho[t] * delta)
        if mutant == "rho_twice":
            rd = f32(rho[t] * rd)
        uc = u1 if mutant == "no_cw" else f32(u1 * cw[t])
        u2 = f32(uc * acc)
        acc = f32(rd + u2)
        acc = f32(acc * keep[t])
        ret[t] = f32(acc + V[t])
        p = f32(A + V[t])
        adv[t] = f32(p - V[t])
    return ret, adv, V, rho


def wave_sum_d(lanes):
    """The double-precision shuffle tree: v += shfl_xor(v, o) for o = 32 .. 1 over 64 lanes (every lane ends with one value)."""
    v = np.asarray(lanes, f64).copy()
    o = 32
    while o:
        v = v + v[np.arange(64) ^ o]
        o >>= 1
    assert (v == v[0]).all()
    return v[0]


def lane_sums(x):
    """Per lane l the sequential double sum of x[l], x[l + 64], ..."""
    out = np.zeros(64, f64)
    for i, v in enumerate(np.asarray(x, f64)):
        out[i % 64] = out[i % 64] + v
    return out


def finish32(a, rho, normalise):
    """The last stage: a_t normalised as gae_multi_kernel normalises, then times rho_t."""
    a, rho = np.asarray(a, f32), np.asarray(rho, f32)
    T = len(a)
    if not normalise:
        return (a * rho).astype(f32)
    mean = wave_sum_d(lane_sums(a)) / T
    d = a.astype(f64) - mean
    sq = wave_sum_d(lane_sums(d * d))
    meanf = f32(mean)
    stdf = f32(np.sqrt(sq / (T - 1)))
    den = f32(stdf + f32(1e-8))
    an = ((a - meanf).astype(f32) / den).astype(f32)
    return (an * rho).astype(f32)


def vtrace32(r, V, m, keep, ratio, boot_keep, gamma, gamma_tau, rho_bar, c_bar, normalise, scale=None, clip=None, mutant=None):
    """The whole kernel for one storage: (returns, advantages, V[T])."""
    ret, a, V2, rho = scan32(r, V, m, keep, ratio, boot_keep, gamma, gamma_tau, rho_bar, c_bar, scale, clip, mutant)
    return ret, finish32(a, rho, normalise), V2[len(ratio)]


def vtrace64(r, V, m, keep, ratio, boot_keep, gamma, lam, rho_bar, c_bar):
    """Float64 V-trace: v_s - V_s = keep_s (rho_s delta_s + gamma lam m_s c_s (v_{s+1} - V_{s+1})) and the policy advantage
    A_s = keep_s (delta_s + gamma lam m_s (v_{s+1} - V_{s+1})).  Returns (v [T], A [T], rho [T])."""
    T = len(ratio)
    r, V, m, ratio = (np.asarray(x, f64) for x in (r, V, m, ratio))
    V = V.copy()
    keep = np.ones(T + 1) if keep is None else np.asarray(keep, f64)
    V[T] = V[T] if boot_keep != 0 else 0.0
    rho, cw = np.minimum(rho_bar, ratio), np.minimum(c_bar, ratio)
    vs, A = np.zeros(T), np.zeros(T)
    nxt = 0.0                                        # v_{s+1} - V_{s+1}
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * V[t + 1] * m[t] - V[t]
        A[t] = keep[t] * (delta + gamma * lam * m[t] * nxt)
        nxt = keep[t] * (rho[t] * delta + gamma * lam * m[t] * cw[t] * nxt)
        vs[t] = nxt + V[t]
    return vs, A, rho


def finish64(A, rho, normalise):
    A, rho = np.asarray(A, f64), np.asarray(rho, f64)
    if not normalise:
        return A * rho
    return (A - A.mean()) / (A.std(ddof=1) + 1e-8) * rho


def diag64(lr, ratio, rho_bar):
    """The four diagnostics in float64 from the fp32 log-ratio differences and the (stored) fp32 ratios."""
    lr, ratio = np.asarray(lr, f64), np.asarray(ratio, f64)
    rho = np.minimum(f64(f32(rho_bar)), ratio)
    T = len(ratio)
    return np.array([ratio.sum() / T, float((ratio > f64(f32(rho_bar))).sum()) / T, np.abs(lr).max(),
                     rho.sum() ** 2 / (T * (rho * rho).sum())])


def ulps32(got, want64):
    """|got - want| in units of the fp32 ulp of want (2^-23 |want|, floored at the smallest normal)."""
    want64 = np.asarray(want64, f64)
    return np.abs(np.asarray(got, f64) - want64) / (2.0 ** -23 * np.maximum(np.abs(want64), 2.0 ** -126))
