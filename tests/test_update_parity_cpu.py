"""The update parity bound of tests/update_parity.py has teeth: it ACCEPTS fp32 numpy emulations of the six fused update kernels' arithmetic
(strictly sequential, and in the kernels' own shape: partial sums of 4 along K, two alternating accumulators, the backward's four quarters of
the gate axis added as (q0 + q1) + (q2 + q3)) and REJECTS every CPU-made mutant.  Every mutant prints the metric of the fused-kernel tests in
tests/test_kernels_gpu.py (max|got - ref| / max|ref| against the chained float64 reference, bar 1e-5 forward / 2e-5 elsewhere) next to the
verdict of the new bound; at least two mutants pass the old bar (asserted).  Small shapes (D = 37, towers 37 -> 16 -> 16 -> 8).  No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import update_parity as up

REJECTED = "excess|no exact zeros|outside its enclosure|not bit-identical"     # the bound's own verdicts (not "the helper is wrong")
ORDERS = ["seq", "kernel"]
D, B = 37, 24
OLD = {}                                                # mutant -> (old metric, old bar): filled by the mutant tests, read by the last test


def rel(a, b):
    return up.old_metric(a, b)


# ----------------------------------------------------------------------------- the helper's own pieces
def test_enclosure_accepts_correctly_rounded_sigmoid_and_tanh():
    """np.float32 of float64 sigmoid / tanh at arguments that are exact in float64 (delta = 0): inside T ulps + the floor, from -110 to 110
    and around 0; a result 8 ulps off is outside."""
    r = np.random.RandomState(0)
    x = np.concatenate([np.linspace(-110, 110, 4001), up.log_uniform(r, 4000, -30, 1), [0.0, -0.0]]).astype(np.float32).astype(np.float64)
    for name, fn, T in (("sigmoid", up.sig64, up.T_ACT), ("tanh", up.tanh64, up.T_TANH)):
        c = up.Case("self-check")
        c.add_enclosure(name, fn(x).astype(np.float32), fn(x), fn(x), T, np.ones(x.shape, bool), fn(x))
        st = c.finish()
        assert st[name][0] <= 0.5 and st[name][2] <= 0.5                  # (half an ulp: the rounding to fp32 itself)
        bad = up.Case("self-check 8 ulp")
        bad.add_enclosure(name, (fn(x) * (1 + 8 * up.ULP)).astype(np.float32), fn(x), fn(x), T)
        with pytest.raises(AssertionError, match="outside its enclosure"):
            bad.finish()


def test_value_magnitude_evaluator_is_the_autograd_of_the_cell():
    """cell_bwd on (value, magnitude) pairs: the values are torch autograd of nn.LSTMCell's cell math in float64 to 1e-12; the magnitudes
    bound the values and follow the rules (mag(1 - x x) = 1 + x x)."""
    g = torch.Generator().manual_seed(3)
    n = 64
    pre = (torch.randn(n, 4 * D, generator=g, dtype=torch.float64) * 2).requires_grad_()
    cp = torch.randn(n, D, generator=g, dtype=torch.float64).requires_grad_()
    dh, dc = torch.randn(n, D, generator=g, dtype=torch.float64), torch.randn(n, D, generator=g, dtype=torch.float64)
    i, f, gg, o = pre.chunk(4, -1)
    si, sf, tg, so = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    c = sf * cp + si * tg
    tc = torch.tanh(c)
    ((so * tc) * dh + c * dc).sum().backward()
    mag_dh = dh.abs().numpy() * 1.5
    outs = up.cell_bwd(up.VM(dh.numpy(), mag_dh), *[up.VM(t.detach().numpy()) for t in (dc, si, sf, tg, so, tc, cp)])
    want = list(pre.grad.chunk(4, -1)) + [cp.grad]
    for o_, w in zip(outs, want):
        assert float(np.abs(o_.v - w.numpy()).max()) <= 1e-12
        assert (o_.m >= np.abs(o_.v)).all()
    x = up.VM(np.array([0.5, -1.0]))
    assert np.array_equal((1.0 - x * x).m, [1.25, 2.0]) and np.array_equal((1.0 - x * x).v, [0.75, 0.0])
    assert np.array_equal((x - x).m, [1.0, 2.0])


# ----------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def fwd_ops():
    return tuple(t[0] for t in up.lstm_fwd_operands(np.random.RandomState(11), 1, B, D, True))


def fwd_ref64():
    """The chained float64 reference of test_lstm_step_fwd_fused -> dict(act, c, tc, h)."""
    W, b, Gx, hp, cp = (up.f64(t) for t in fwd_ops())
    pre = Gx + hp @ W.t() + b
    i, f, g, o = pre.chunk(4, -1)
    act = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], -1)
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(g)
    return dict(act=act, c=c, tc=torch.tanh(c), h=torch.sigmoid(o) * torch.tanh(c))


def fwd_verdict(got, what):
    case = up.Case(what)
    up.lstm_fwd_check(case, *fwd_ops(), got)
    return case.finish()


def fwd_old(got):
    ref = fwd_ref64()
    return max(rel(got[k], ref[k]) for k in ("act", "c", "tc", "h")), 1e-5


@functools.lru_cache(maxsize=None)
def bwd_ops():
    r = np.random.RandomState(12)
    W = torch.from_numpy(r.standard_normal((4 * D, D)).astype(np.float32) * np.float32(0.15))
    dG_t, dh_in, dc, cp, tc, act = (t[0] for t in up.lstm_bwd_operands(r, 1, B, D, True))
    return W, dG_t, dh_in, act, tc, cp, dc


def bwd_verdict(got, with_product, what):
    case = up.Case(what)
    up.lstm_bwd_check(case, *bwd_ops(), got[0], got[1], with_product)
    return case.finish()


def bwd_old(got, with_product):
    """test_lstm_step_bwd_fused's figure: dG and dc each against the largest element of its float64 reference."""
    W, dG_t, dh_in, act, tc, cp, dc = (up.f64(t) for t in bwd_ops())
    dh = (dG_t @ W if with_product else 0) + dh_in
    outs = up.cell_bwd(dh, dc, *act.view(-1, 4, D).unbind(1), tc, cp)
    return max(rel(got[0], torch.cat(outs[:4], 1)), rel(got[1], outs[4])), 2e-5


@functools.lru_cache(maxsize=None)
def dw_ops():
    """One net of cadre_lstm_dw: S = 3 steps of a 7-row run inside B = 9 (rows 1 .. 7), H4 = 20 gate columns, two second operands of 12
    columns (h and x).  -> (dG [S][B][H4], [Hs, X] [S][B][12], run)."""
    r = np.random.RandomState(13)
    return torch.from_numpy(r.standard_normal((3, 9, 20)).astype(np.float32)), \
        [torch.from_numpy(r.standard_normal((3, 9, 12)).astype(np.float32)) for _ in range(2)], (1, 7)


def dw_rows(rows):
    dG, Ys, _ = dw_ops()
    return dG[:, rows].reshape(-1, 20), [Y[:, rows].reshape(-1, 12) for Y in Ys]


def dw_verdict(got, what):
    lo, n = dw_ops()[2]
    dY, Ys = dw_rows(slice(lo, lo + n))
    case = up.Case(what)
    up.dw_check(case, "dW_hh, dW_ih, db", dY, Ys, got[0], got[1])
    return case.finish()


def dw_old(got):
    lo, n = dw_ops()[2]
    dY, Ys = dw_rows(slice(lo, lo + n))
    return max([rel(w, up.f64(dY).t() @ up.f64(Y)) for w, Y in zip(got[0], Ys)] + [rel(got[1], up.f64(dY).sum(0))]), 2e-5


HID, NP, NOUT, NR = 16, 8, (5, 1), 17


@functools.lru_cache(maxsize=None)
def mlp_ops():
    """One net: H [NR][D], its two towers' parameters (W3 / b3 rows past n_out zero, as the update's padded towers), dO3 [2][NR][NP]."""
    r = np.random.RandomState(14)
    rn = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    H = rn(NR, D)
    P, dO3 = [], torch.zeros(2, NR, NP)
    for tw in range(2):
        W3, b3 = torch.zeros(NP, HID), torch.zeros(NP)
        W3[:NOUT[tw]], b3[:NOUT[tw]] = rn(NOUT[tw], HID) * 0.3, rn(NOUT[tw]) * 0.1
        P.append((rn(HID, D) * 0.2, rn(HID) * 0.1, rn(HID, HID) * 0.3, rn(HID) * 0.1, W3, b3))
        dO3[tw, :, :NOUT[tw]] = rn(NR, NOUT[tw]) * 0.3
    return H, P, dO3


def mlp_ref64():
    """The chained float64 autograd reference of test_mlp_towers_fused -> (forward tensors per tower, dH, parameter gradients per tower)."""
    H, P, dO3 = mlp_ops()
    Hd = up.f64(H).requires_grad_()
    fw = []
    loss = 0
    Pd = [[up.f64(t).requires_grad_() for t in p] for p in P]
    for tw in range(2):
        W1, b1, W2, b2, W3, b3 = Pd[tw]
        a1 = torch.relu(Hd @ W1.t() + b1)
        a2 = torch.relu(a1 @ W2.t() + b2)
        o3 = a2 @ W3.t() + b3
        fw.append(dict(A1=a1.detach(), A2=a2.detach(), O3=o3.detach()))
        loss = loss + (o3 * up.f64(dO3[tw])).sum()
    loss.backward()
    return fw, Hd.grad, [[t.grad for t in p] for p in Pd]


def mlp_run(order="seq", quant=None, **bwd_kw):
    """The three kernels' emulation on one net, each stage on the previous one's stored results."""
    H, P, dO3 = mlp_ops()
    fw = [up.mlp_fwd_emulate(H, P[tw], order, quant) for tw in range(2)]
    A1, A2 = torch.stack([f["A1"] for f in fw]), torch.stack([f["A2"] for f in fw])
    bw = up.mlp_bwd_emulate(dO3, A1, A2, P[0], P[1], order, **bwd_kw)
    dw = []
    for tw in range(2):
        (w1,), d1 = up.dw_emulate(bw["dA1"][tw], [H], order)
        (w2,), d2 = up.dw_emulate(bw["dA2"][tw], [A1[tw]], order)
        (w3,), d3 = up.dw_emulate(dO3[tw], [A2[tw]], order)
        dw.append((w1, d1, w2, d2, w3, d3))
    return fw, A1, A2, bw, dw


def mlp_verdict(run, what):
    H, P, dO3 = mlp_ops()
    fw, A1, A2, bw, dw = run
    case = up.Case(what)
    for tw in range(2):
        up.mlp_fwd_check(case, H, P[tw], fw[tw])
    up.mlp_bwd_check(case, dO3, A1, A2, P[0], P[1], bw)
    for tw in range(2):
        up.mlp_dw_check(case, dO3[tw], bw["dA2"][tw], bw["dA1"][tw], A2[tw], A1[tw], H, dw[tw])
    return case.finish()


def mlp_old(run):
    fw, A1, A2, bw, dw = run
    rf, rh, rg = mlp_ref64()
    e = [rel(fw[tw][k], rf[tw][k]) for tw in range(2) for k in ("A1", "A2", "O3")] + [rel(bw["dH"], rh)]
    e += [rel(g, w) for tw in range(2) for g, w in zip(dw[tw], rg[tw])]
    return max(e), 2e-5


# ----------------------------------------------------------------------------- honest emulations are accepted
@pytest.mark.parametrize("order", ORDERS)
def test_forward_step_emulation_accepted(order):
    got = up.lstm_fwd_emulate(*fwd_ops(), order=order)
    st = fwd_verdict(got, "lstm_step_fwd emulation %s" % order)
    print("old metric %.2e (bar %.0e)" % fwd_old(got))
    assert st["sigmoid gates"][2] <= 0.5 and st["tanh(c_t)"][2] <= 0.5          # correctly rounded where the argument is known
    assert fwd_old(got)[0] < 1e-5


@pytest.mark.parametrize("with_product", [1, 0])
@pytest.mark.parametrize("right,fma", up.POLY_ORDERS)
@pytest.mark.parametrize("order", ORDERS)
def test_backward_step_emulation_accepted(order, right, fma, with_product):
    W, dG_t, dh_in, act, tc, cp, dc = bwd_ops()
    got = up.lstm_bwd_emulate(W, dG_t, dh_in, act, tc, cp, dc, with_product, order, right, fma)
    bwd_verdict(got, with_product, "lstm_step_bwd emulation %s right %d fma %d product %d" % (order, right, fma, with_product))
    assert bwd_old(got, with_product)[0] < 2e-5


@pytest.mark.parametrize("order", ORDERS)
def test_dw_emulation_accepted(order):
    lo, n = dw_ops()[2]
    got = up.dw_emulate(*dw_rows(slice(lo, lo + n)), order=order)
    dw_verdict(got, "lstm_dw emulation %s" % order)
    assert dw_old(got)[0] < 2e-5
    case = up.Case("lstm_dw empty run")                                            # a net without rows: exact zeros, and nothing else
    up.dw_check(case, "dW, db", *dw_rows(slice(0, 0)), *up.dw_emulate(*dw_rows(slice(0, 0))))
    case.finish()
    bad = up.Case("lstm_dw empty run, stale gradient")
    w, b_ = up.dw_emulate(*dw_rows(slice(0, 0)))
    w[0][3, 4] = 1e-30
    up.dw_check(bad, "dW, db", *dw_rows(slice(0, 0)), w, b_)
    with pytest.raises(AssertionError, match="no exact zeros"):
        bad.finish()


@pytest.mark.parametrize("order", ORDERS)
def test_mlp_emulation_accepted(order):
    run = mlp_run(order)
    mlp_verdict(run, "mlp towers emulation %s" % order)
    assert mlp_old(run)[0] < 2e-5


# ----------------------------------------------------------------------------- mutants are rejected
def _mutant(name, verdict, old):
    """The new bound must reject; the old metric is recorded next to it."""
    with pytest.raises(AssertionError, match=REJECTED) as e:
        verdict()
    OLD[name] = old
    print("MUTANT %-44s old metric %.2e (bar %.0e): old bar %s; new bound rejects: %s"
          % (name, old[0], old[1], "ACCEPTS" if old[0] < old[1] else "rejects", str(e.value)[:160]))


FWD_MUTANTS = {
    "tanh as 2 sigmoid(2x) - 1": dict(tanh=up.tanh_by_sigmoid32),
    "sigmoid from an exp 2^-18 off": dict(sig=up.sig_rough_exp32),
    "forward operands cut to 10 mantissa bits": dict(quant=up.trunc_mantissa),
    "bias added to three gates only": dict(bias_gates=3),
}


@pytest.mark.parametrize("name", list(FWD_MUTANTS))
def test_forward_step_mutant_rejected(name):
    got = up.lstm_fwd_emulate(*fwd_ops(), order="kernel", **FWD_MUTANTS[name])
    _mutant(name, lambda: fwd_verdict(got, name), fwd_old(got))


def _c_t():
    W, dG_t, dh_in, act, tc, cp, dc = bwd_ops()
    ig, fg, gg, og = act.view(-1, 4, D).unbind(1)
    return fg * cp + ig * gg


BWD_MUTANTS = {
    "f-gate gradient from c_t for c_{t-1}": dict(cp_f=_c_t),
    "(1 - tc) for (1 - tc tc)": dict(lin_tc=True),
    "backward operands cut to 10 mantissa bits": dict(quant=up.trunc_mantissa),
}


@pytest.mark.parametrize("name", list(BWD_MUTANTS))
def test_backward_step_mutant_rejected(name):
    kw = {k: (v() if k == "cp_f" else v) for k, v in BWD_MUTANTS[name].items()}
    got = up.lstm_bwd_emulate(*bwd_ops(), 1, "kernel", **kw)
    _mutant(name, lambda: bwd_verdict(got, 1, name), bwd_old(got, 1))


@pytest.mark.parametrize("name,rows,quant", [("dw tail: the run's last row dropped", slice(1, 7), None),
                                             ("dw tail: one foreign row included", slice(1, 9), None),
                                             ("dw operands cut to 10 mantissa bits", slice(1, 8), up.trunc_mantissa)])
def test_dw_mutant_rejected(name, rows, quant):
    got = up.dw_emulate(*dw_rows(rows), order="kernel", quant=quant)
    _mutant(name, lambda: dw_verdict(got, name), dw_old(got))


MLP_MUTANTS = {
    "dH from one tower only": dict(towers=(0,)),
    "ReLU mask >= 0 for > 0": dict(mask=lambda a: a >= 0),
    "tower operands cut to 10 mantissa bits": dict(quant=up.trunc_mantissa),
}


@pytest.mark.parametrize("name", list(MLP_MUTANTS))
def test_mlp_mutant_rejected(name):
    run = mlp_run("kernel", **MLP_MUTANTS[name])
    _mutant(name, lambda: mlp_verdict(run, name), mlp_old(run))


def test_at_least_two_mutants_pass_the_old_bar():
    """Every mutant again (the table does not depend on which tests ran before), then: at least two that the new bound rejects lie under
    the old bar."""
    for name in FWD_MUTANTS:
        test_forward_step_mutant_rejected(name)
    for name in BWD_MUTANTS:
        test_backward_step_mutant_rejected(name)
    test_dw_mutant_rejected("dw tail: the run's last row dropped", slice(1, 7), None)
    test_dw_mutant_rejected("dw tail: one foreign row included", slice(1, 9), None)
    test_dw_mutant_rejected("dw operands cut to 10 mantissa bits", slice(1, 8), up.trunc_mantissa)
    for name in MLP_MUTANTS:
        test_mlp_mutant_rejected(name)
    passed = sorted(n for n, (m, bar) in OLD.items() if m < bar)
    print("mutants under the old bar that the new bound rejects: %s" % passed)
    assert len(OLD) == 13 and len(passed) >= 2, passed
