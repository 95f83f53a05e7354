"""No GPU: the bound of tests/attention_parity.py has teeth and admits the honest orders.

  * the float64 bodies of the helper are oracle/encoder_ref.py's pam / cam run in float64 and the `cross` formula of
    test_kernels_gpu.py::test_intertask_tail_and_measurements in float64, to float64 rounding: the bound is laid around the right function;
  * the fp32 numpy emulation of every body passes every bound at every case of the GPU file (1024 positions: the benign family), in two
    orders (the kernels' — ascending k chains, strided lane sums and the shuffle tree — and strictly sequential sums with the chains the
    other way round); the worst err / bound is printed;
  * no case has an ambiguous row and every c_bar is under its cap (asserted where the reference is built: attention_parity.reference);
  * the bound is not vacuous: on the benign family up to 128 positions the largest bound of a frame is at most the old bar's absolute
    tolerance 2e-5 max|y64|; for the other families the median and the maximum of bound / (2^-24 |y64|) are printed;
  * every one-statement mutant fails the bound on at least one case; whether it passes the OLD bar (max|got - ref| / max|ref| < 2e-5 on the
    benign family at the old tests' sizes) is printed next to it ("attention parity")."""
import numpy as np
import pytest
import torch

from tests import attention_parity as ap
from tests.attention_parity import F4, F8, U, X32, X64, Report

MUTANT_SIZES = (3, 33, 65, 129)


def _judge(got, ref, what):
    """-> (fails the bound, worst err / bound or inf where an output is not finite or a zero-bound element is not exact)."""
    rep = Report(what)
    rep.check("y", got, ref["y"])
    return bool(rep.bad), (float("inf") if rep.bad and rep.worst <= 1.0 else rep.worst)


# ----------------------------------------------------------------------------- the reference is the right function
@pytest.mark.parametrize("h,w,scale", [(1, 3, 0.1), (3, 11, 0.1), (5, 8, 1.0), (9, 9, 0.5)])
def test_float64_pam_and_cam_bodies_equal_the_oracle(h, w, scale):
    from oracle import encoder_ref
    r = np.random.RandomState(h * 100 + w)
    Np, Fn = h * w, 2
    x = np.stack([0.4 * r.standard_normal((Np, 128)), ap._relu_frame(r, Np)])                 # [F][Np][128]
    W, b = scale * r.standard_normal((160, 128)), 0.1 * r.standard_normal(160)
    sd = {"da_head.sa.gamma": torch.tensor([0.5], dtype=torch.float64), "da_head.sc.gamma": torch.tensor([float(ap.GAMMA_CAM)], dtype=torch.float64)}
    for nm, sl in (("query", slice(0, 16)), ("key", slice(16, 32)), ("value", slice(32, 160))):
        sd["da_head.sa.%s_conv.weight" % nm] = torch.from_numpy(W[sl].reshape(-1, 128, 1, 1).copy())
        sd["da_head.sa.%s_conv.bias" % nm] = torch.from_numpy(b[sl].copy())
    xt = torch.from_numpy(x.reshape(Fn, h, w, 128).transpose(0, 3, 1, 2).copy())
    want_p = encoder_ref.pam(xt, sd).permute(0, 2, 3, 1).reshape(Fn, Np, 128).numpy()
    want_c = encoder_ref.cam(xt, sd).permute(0, 2, 3, 1).reshape(Fn, Np, 128).numpy()
    X = X64()
    for f in range(Fn):
        qkv = x[f] @ W.T + b
        got_p = ap.pam_row(X, qkv[:, :16], qkv[:, 16:32], qkv[:, 32:], x[f], 0.5, {})
        got_c = ap.cam_row(X, x[f], ap.GAMMA_CAM, {})
        assert np.abs(got_p - want_p[f]).max() <= 1e-12 * np.abs(want_p[f]).max()
        assert np.abs(got_c - want_c[f]).max() <= 1e-12 * np.abs(want_c[f]).max()


@pytest.mark.parametrize("fams,temp", ap.it_keys())
def test_float64_intertask_body_equals_the_cross_formula(fams, temp):
    c, _ = ap.it_case(fams, temp)
    Fn = c.F
    vq, vk, vv, bq, bk, bv = (torch.from_numpy(c.qkv[:, i].astype(F8)) for i in range(6))

    def cross(q, k, v):
        e = torch.bmm((q.view(Fn, 1, 256).permute(0, 2, 1)) / float(F4(temp)), k.view(Fn, 1, 256))
        att = torch.softmax(e, -1)
        return torch.bmm(v.view(Fn, 1, 256), att.permute(0, 2, 1)).view(Fn, -1) + v
    want = torch.cat([cross(bq, vk, vv), cross(vq, bk, bv)], -1).numpy()
    got = ap.run_it(c, X64())
    assert got.shape == (Fn, 512)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ----------------------------------------------------------------------------- honest orders inside
def _cpu_keys(kind):
    return [k for k in ap.case_keys(kind) if k[1] != ap.BIG or k[2] == ("benign",)]


@pytest.mark.parametrize("kind", ["pam", "cam"])
def test_honest_emulations_pass_every_bound(kind):
    worst = {"tree": 0.0, "seq": 0.0}
    for key in _cpu_keys(kind):
        c, ref = ap.att_case(*key)
        for name, per_frame in ref["cb"].items():
            for cb, cap, chains in per_frame:
                assert 0 <= cb <= cap, (c.tag(), name)
        for order in ("tree", "seq"):
            got = ref["emu"] if order == "tree" else ap.run_att(c, X32("seq"))
            worst[order] = max(worst[order], ap.check_att(got, ref, "%s, %s order" % (c.tag(), order), quiet=True))
        print("%s: c_bar per frame: energy %s (cap %d), product %s (cap %d)"
              % (c.tag(), " ".join("%.2f" % t[0] for t in ref["cb"]["energy"]), ref["cb"]["energy"][0][1],
                 " ".join("%.2f" % t[0] for t in ref["cb"]["product"]), ref["cb"]["product"][0][1]))
    print("%s emulation, worst err / bound: kernels' order %.3f, sequential %.3f" % (kind, worst["tree"], worst["seq"]))


def test_honest_intertask_emulations_pass_every_bound():
    for key in ap.it_keys():
        c, ref = ap.it_case(*key)
        for order in ("tree", "seq"):
            ap.check_att(ap.run_it(c, X32(order)), ref, "%s, %s order" % (c.tag(), order))


# ----------------------------------------------------------------------------- the bound is not vacuous
@pytest.mark.parametrize("kind", ["pam", "cam"])
def test_bound_is_below_the_old_bar_on_the_old_inputs(kind):
    for key in _cpu_keys(kind):
        c, ref = ap.att_case(*key)
        for f, fam in enumerate(c.fams):
            y, e = ref["y"].v[f], ref["y"].e[f]
            if fam == "benign" and c.Np <= 128:
                tol = 2e-5 * np.abs(y).max()
                print("%s frame %d benign: largest bound %.3g, old tolerance %.3g (x %.1f)" % (c.tag(), f, e.max(), tol, tol / e.max()))
                assert e.max() <= tol, c.tag()
            elif (y != 0).any():
                live = y != 0
                q = e[live] / (U * np.abs(y[live]))
                print("%s frame %d %s: bound / (2^-24 |y64|) median %.1f, max %.3g" % (c.tag(), f, fam, np.median(q), q.max()))


def test_intertask_bound_is_below_the_old_bar_on_the_old_inputs():
    for key in ap.it_keys():
        c, ref = ap.it_case(*key)
        for f, fam in enumerate(c.fams):
            y, e = ref["y"].v[f], ref["y"].e[f]
            q = e / (U * np.abs(y))
            print("%s frame %d %s: bound / (2^-24 |y64|) median %.1f, max %.3g" % (c.tag(), f, fam, np.median(q), q.max()))
            if fam == "benign":
                tol = 2e-5 * np.abs(y).max()
                print("    largest bound %.3g, old tolerance %.3g (x %.1f)" % (e.max(), tol, tol / e.max()))
                assert e.max() <= tol, c.tag()


def test_exact_elements_have_a_zero_bound():
    """An all-zero frame through PAM and CAM, an all-zero position through CAM: bound zero, so the GPU test asks for the bits."""
    for kind in ("pam", "cam"):
        c, ref = ap.att_case(kind, 33, ap.TRIPLES[1])
        f = c.fams.index("zero")
        assert (ref["y"].e[f] == 0).all() and (ref["y"].v[f] == 0).all()
    c, ref = ap.att_case("cam", 33, ap.TRIPLES[1])
    f = c.fams.index("relu")
    assert (ref["y"].e[f][33 // 2] == 0).all() and (ref["y"].e[f] > 0).any()


# ----------------------------------------------------------------------------- mutants
def _old_bar(kind, mut):
    """The old bar on the old input: max|got - ref| / max|ref| over benign frames at the old test's sizes -> worst value."""
    worst = 0.0
    for Np in ap.OLD_SIZES:
        c = ap.AttCase(kind, Np, ("benign",) * 3)
        with np.errstate(all="ignore"):
            got = ap.run_att(c, X32("tree"), mut=(mut,))
        if not np.isfinite(got).all():
            return float("inf")
        worst = max(worst, ap.old_metric(got, ap.run_att(c, X64())))
    return worst


@pytest.mark.parametrize("kind", ["pam", "cam"])
def test_mutants_fail_the_bound(kind):
    keys = [k for k in ap.case_keys(kind, small_only=True) if k[1] in MUTANT_SIZES]
    print()
    for mut in (ap.PAM_MUTANTS if kind == "pam" else ap.CAM_MUTANTS):
        hits, worst, where = 0, 0.0, ""
        for key in keys:
            c, ref = ap.att_case(*key)
            with np.errstate(all="ignore"):
                got = ap.run_att(c, X32("tree"), mut=(mut,))
            bad, w = _judge(got, ref, c.tag())
            hits += bad
            if w > worst:
                worst, where = w, c.tag()
            if mut == "no_max" and kind == "pam":                                # energies of +200: expf overflows without the maximum
                assert not np.isfinite(got[c.fams.index("offset")]).all(), c.tag()
        old = _old_bar(kind, mut)
        print("mutant %-22s %s: fails %2d of %d cases, worst err / bound %.3g (%s); old metric %.3g -> %s the old bar"
              % (mut, kind, hits, len(keys), worst, where, old, "PASSES" if old < 2e-5 else "fails"))
        assert hits >= 1, "%s mutant %s passes the bound on every case" % (kind, mut)


def test_intertask_mutants_fail_the_bound():
    old_c = ap.ItCase(("benign",) * 4, 16.0)
    old_ref = ap.run_it(old_c, X64())
    print()
    for mut in ap.IT_MUTANTS:
        hits, worst = 0, 0.0
        for key in ap.it_keys():
            c, ref = ap.it_case(*key)
            with np.errstate(all="ignore"):
                got = ap.run_it(c, X32("tree"), mut=(mut,))
            bad, w = _judge(got, ref, c.tag())
            hits += bad
            worst = max(worst, w)
        with np.errstate(all="ignore"):
            g = ap.run_it(old_c, X32("tree"), mut=(mut,))
        old = ap.old_metric(g, old_ref) if np.isfinite(g).all() else float("inf")
        print("mutant %-22s intertask: fails %d of %d cases, worst err / bound %.3g; old metric %.3g -> %s the old bar"
              % (mut, hits, len(ap.it_keys()), worst, old, "PASSES" if old < 2e-5 else "fails"))
        assert hits >= 1, "inter-task mutant %s passes the bound on every case" % mut
