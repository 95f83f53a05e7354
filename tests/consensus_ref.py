"""Host mirrors of the two rank-consensus kernels (csrc/consensus.hip, csrc/kl_rule.h), independent of the package: the KL
rule in numpy float32 / float64 exactly as the device types it, and Chan's merge of per-rank (count, mean, M2) in rank order.
Shared by tests/test_consensus_cpu.py and tests/test_consensus_gpu.py."""
import numpy as np

F32, F64 = np.float32, np.float64
HP_LR, HP_DESIRED_KL, HP_LR_MIN, HP_LR_MAX, HP_LR_FACTOR = 0, 6, 7, 8, 9


def kl_rule(kl, target_kl, stop, desired, hp):
    """kl: the two float32 KL values; stop: the flag before the step (0 / 1), or None when the caller has no flag;
    hp: float64 block (only LR, LR_MIN, LR_MAX, LR_FACTOR are read), or None.  Returns (stop after, applied, lr after):
    np.fmax is C's fmaxf / fmax (a NaN operand is ignored), every comparison with NaN is false."""
    kl0, kl1, target_kl = F32(kl[0]), F32(kl[1]), F32(target_kl)
    stopped = 0 if stop is None else int(stop)
    with np.errstate(invalid="ignore"):
        if stop is not None and target_kl > F32(0) and np.fmax(kl0, kl1) > F32(1.5) * target_kl:
            stopped = 1
        lr = None if hp is None else F64(hp[HP_LR])
        desired = F64(desired)
        if hp is not None and desired > 0.0 and not stopped:
            k = np.fmax(F64(kl0), F64(kl1))
            if k > F64(2.0) * desired:
                lr = np.fmax(F64(hp[HP_LR_MIN]), lr / F64(hp[HP_LR_FACTOR]))
            elif k > 0.0 and k < desired / F64(2.0):
                lr = np.fmin(F64(hp[HP_LR_MAX]), lr * F64(hp[HP_LR_FACTOR]))
    return stopped, (0.0 if stopped else 1.0), lr


LR0, LR_MIN, LR_MAX, FACTOR = 3e-4, 2.5e-4, 4e-4, 1.5


def hp_block(lr=LR0, lr_min=LR_MIN, lr_max=LR_MAX, factor=FACTOR, fill=0.0):
    hp = np.full(16, fill, dtype=np.float64)
    hp[HP_LR], hp[HP_LR_MIN], hp[HP_LR_MAX], hp[HP_LR_FACTOR] = lr, lr_min, lr_max, factor
    return hp


def decision_table():
    """(name, kl pair, target_kl, stop before (None: no flag), desired_kl, lr before) — the cases of the issue.  The
    threshold 1.5f * target is formed in float32, and the neighbours of it are taken with nextafter."""
    t = F32(0.02)
    thr = F32(1.5) * t
    below, above = np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1))
    d = 0.01
    nan = F32("nan")
    return [
        ("just below 1.5 target", (below, F32(0.001)), t, 0, 0.0, LR0),
        ("exactly at 1.5 target (strict >)", (F32(0.001), thr), t, 0, 0.0, LR0),
        ("just above 1.5 target", (above, F32(0.0)), t, 0, 0.0, LR0),
        ("above, throttle head", (F32(0.0), above), t, 0, d, LR0),
        ("flag already set: stays set, lr untouched", (F32(1e-5), F32(1e-5)), t, 1, d, LR0),
        ("flag already set, kl far above 2 desired", (F32(0.5), F32(0.5)), t, 1, d, LR0),
        ("target 0: no check", (F32(10.0), F32(10.0)), F32(0.0), 0, 0.0, LR0),
        ("target 0 without a flag", (F32(10.0), F32(10.0)), F32(0.0), None, d, LR0),
        ("desired 0: lr stays", (F32(0.025), F32(0.001)), t, 0, 0.0, LR0),
        ("kl > 2 desired: lr / factor", (F32(0.021), F32(0.001)), t, 0, d, 3.9e-4),
        ("kl > 2 desired: down to lr_min", (F32(0.021), F32(0.001)), t, 0, d, LR0),
        ("kl == 2 desired: stays (strict >)", (F32(F64(F32(0.02))), F32(0.0)), F32(1.0), 0, float(F64(F32(0.02))) / 2.0, LR0),
        ("0 < kl < desired / 2: lr * factor", (F32(0.001), F32(0.004)), t, 0, d, 2.6e-4),
        ("0 < kl < desired / 2: up to lr_max", (F32(0.001), F32(0.004)), t, 0, d, LR0),
        ("kl == 0: stays", (F32(0.0), F32(0.0)), t, 0, d, LR0),
        ("negative kl (rounding): stays", (F32(-1e-9), F32(-2e-9)), t, 0, d, LR0),
        ("NaN in both heads: no stop, lr stays", (nan, nan), t, 0, d, LR0),
        ("NaN in one head: the other decides", (nan, above), t, 0, d, LR0),
        ("NaN in one head, small other: lr up", (F32(0.001), nan), t, 0, d, 2.6e-4),
        ("gate fires and lr would move: lr stays", (above, above), t, 0, 1e-3, LR0),
    ]


def chan_merge(stats):
    """stats [world][6] float64: per rank (count, mean, M2) of head 0 then head 1.  Returns merged [6]: Chan's formula in
    rank order from an empty accumulator, ranks with count 0 skipped — the statement order of the kernel."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 6)
    out = np.zeros(6, dtype=np.float64)
    for h in range(2):
        cnt = mu = m2 = F64(0.0)
        for r in range(stats.shape[0]):
            nb, mk, qk = stats[r, 3 * h:3 * h + 3]
            if not nb > 0.0:
                continue
            tot = cnt + nb
            delta = mk - mu
            mu = mu + delta * nb / tot
            m2 = m2 + qk + delta * delta * cnt * nb / tot
            cnt = tot
        out[3 * h:3 * h + 3] = cnt, mu, m2
    return out


def scale_of(merged, epsilon):
    """The two float32 scales of a merged block; None where the count is 0 (the kernel then leaves the slot alone)."""
    return [None if merged[3 * h] <= 0 else F32(1.0 / np.sqrt(merged[3 * h + 2] / merged[3 * h] + F64(epsilon))) for h in range(2)]


def rank_stats(data):
    """data: per rank a pair (head 0 samples, head 1 samples) of 1-d float64 arrays (possibly empty) -> stats [world][6]."""
    rows = []
    for pair in data:
        row = []
        for x in pair:
            x = np.asarray(x, dtype=np.float64)
            row += [float(x.size), float(x.mean()) if x.size else 0.0, float(((x - x.mean()) ** 2).sum()) if x.size else 0.0]
        rows.append(row)
    return np.array(rows, dtype=np.float64)


def merge_cases():
    """world 1, 2 and 5; one rank of the world-5 case (and one head of a world-2 rank) has count 0."""
    r = np.random.RandomState(5)
    mk = lambda n, loc, sc: r.standard_normal(n) * sc + loc
    return {
        1: [(mk(16, 0.3, 2.0), mk(16, -4.0, 0.5))],
        2: [(mk(48, 1.0, 3.0), mk(48, 100.0, 1e-2)), (mk(16, -2.0, 0.1), np.zeros(0))],
        5: [(mk(16, 0.0, 1.0), mk(16, 5.0, 2.0)), (np.zeros(0), np.zeros(0)), (mk(32, 3.0, 0.5), mk(32, 5.5, 1.0)),
            (mk(64, -1.0, 4.0), mk(64, 4.0, 0.2)), (mk(16, 0.5, 1.0), mk(16, 6.0, 3.0))],
    }
