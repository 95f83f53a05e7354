"""No GPU: the bound of tests/loss_parity.py has teeth and admits the honest orders.

  * the float64 row bodies of the helper are the project's float64 autograd references (tests/ordinal_ref.py, imitation_ref.py,
    demo_mix_ref.py) to float64 rounding: the bound is laid around the right function;
  * the fp32 numpy emulation of every kernel's statements passes every bound at every case of the GPU file, in two summation orders
    (the kernels' shuffle tree / ladder scans, and strictly sequential); the worst err / bound is printed;
  * every case meets at most one ambiguous row (planted ties aside), from the float64 pairs alone; every PPO case with B >= 15 has rows
    clipped above, clipped below and unclipped;
  * the scratch probe of the plain categorical PPO gradient, redone: K = 3 / 33 / 64, logit scale 1 / 4 / 16, 4096 rows each;
  * one-statement mutants fail, and their value in the OLD metric (max|got - ref| / max|ref| on the old tests' own inputs, bars 2e-5 for
    dlogits and 2e-7 absolute for the Adam parameters) is printed next to it: at least three pass the old bars."""
import math

import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests.loss_parity import F4, F8, X32, X64, XVE


@pytest.fixture(scope="module")
def cases():
    return {kind: lp.loss_cases(kind) for kind in ("ppo", "bc", "mix")}


@pytest.fixture(scope="module")
def refs(cases):
    return {kind: [lp.run_loss(c, XVE) for c in cs] for kind, cs in cases.items()}


def _grid(case, buf, ld, ns, n):
    """flat buffer -> [2C][B][n] of the addressed elements."""
    net, b, k = np.meshgrid(np.arange(2 * case.C), np.arange(case.B), np.arange(n), indexing="ij")
    return np.asarray(buf)[net * ns + b * ld + k]


# ----------------------------------------------------------------------------- the reference is the right function
@pytest.mark.parametrize("kind,i", [("ppo", 1), ("ppo", 5), ("ppo", 8), ("bc", 1), ("bc", 2), ("mix", 0), ("mix", 1), ("mix", 2)])
def test_float64_bodies_equal_the_autograd_references(cases, kind, i):
    from tests import demo_mix_ref, imitation_ref
    c = cases[kind][i]
    hp = {k: float(v) for k, v in c.hp.items()}
    lg = torch.from_numpy(_grid(c, c.logits, c.ldl, c.l_ns, c.ldl).astype(F8)).requires_grad_(True)
    vv = torch.from_numpy(_grid(c, c.values, c.ldv, c.v_ns, 1)[..., 0].astype(F8)).requires_grad_(True)
    ranks = tuple(None if c.rk(h) is None else c.rk(h).tolist() for h in range(2))
    t = lambda a: torch.from_numpy(np.asarray(a))
    if kind == "bc":
        tv, tb, te, total, dst = imitation_ref.bc_loss(lg, vv, t(c.actions), t(c.cmds), t(c.rets), t(c.weights), c.Ks, ranks, c.C, hp["smoothing"],
                                                       hp["bc_coeff"], hp["value_coeff"], hp["ent_coeff"], hp["inv_b"])
        want = dict(losses=[tv, tb, te], demo_stats=dst)
    else:
        # (PPO rows with a planted tie sit on torch's 0.5 / 0.5 split, as the kernels do)
        out = demo_mix_ref.mixed_loss(lg, vv, t(c.actions), t(c.cmds), t(c.old_v), t(c.rets), t(c.old_lp), t(c.adv), t(c.kindrow), c.Ks, ranks, c.C,
                                      hp["clip"], hp["value_coeff"], hp["clip_coeff"], hp["ent_coeff"], hp["inv_b"], hp["smoothing"],
                                      hp["demo_coeff"], hp["demo_value_coeff"], hp["inv_bd"])
        total = out["total"]
        want = dict(losses=list(out["losses"]), stats=out["stats"])
        if kind == "mix":
            want.update(demo_losses=list(out["demo_losses"]), demo_stats=out["demo_stats"])
    total.backward()
    got, bound = lp.run_loss(c, X64()), lp.run_loss(c, XVE)
    dl = _grid(c, got["dlogits"], c.ldl, c.l_ns, c.ldl)
    dv = _grid(c, got["dvalues"], c.ldv, c.v_ns, 1)[..., 0]
    # An ordinal head: autograd forms sigmoid' as s (1 - s), which has lost 8 of float64's 16 digits at a unit of +20 (the helper forms s t
    # with t = sigmoid(-x)), and tests/ordinal_ref.py adds the double 1e-8 where the kernels and the helper add the float 1e-8f (6e-9 of
    # it apart, which a saturated unit's log shows).  s (1 - s) at x = 20 is 2^-53 / 2e-9 = 5.5e-8 of the element off, the bound there is
    # about 1.5e-6 of it: the two must agree to a twentieth of the bound; without an ordinal head to float64 rounding.
    slack = 0.05 if any(c.ordinal) else 0.0

    def close(g, w, e, name):
        w = np.asarray(w, F8)
        assert (np.abs(np.asarray(g, F8) - w) <= 1e-12 * max(1.0, float(np.abs(w).max())) + slack * np.asarray(e)).all(), name

    close(dl, lg.grad.numpy(), _grid(c, bound["dlogits"].e, c.ldl, c.l_ns, c.ldl), "dlogits")
    close(dv, vv.grad.numpy(), _grid(c, bound["dvalues"].e, c.ldv, c.v_ns, 1)[..., 0], "dvalues")
    for name in ("losses", "demo_losses"):
        if name in want:
            close([float(x) for x in got[name]], [float(torch.as_tensor(x).detach()) for x in want[name]], [float(x.e) for x in bound[name]], name)
    for name in ("stats", "demo_stats"):
        if name in want:
            close(np.stack([np.asarray(x) for x in got[name]], 1), want[name].numpy(), np.stack([x.e for x in bound[name]], 1), name)


# ----------------------------------------------------------------------------- honest orders inside, ambiguity, branches
@pytest.mark.parametrize("kind", ["ppo", "bc", "mix"])
def test_honest_emulations_pass_every_bound(cases, refs, kind):
    for c, ref in zip(cases[kind], refs[kind]):
        for order in ("tree", "seq"):
            _w, n_amb = lp.check_loss(c, lp.emulate_loss(c, order), ref, "%s, %s sums" % (c.tag(), order))
        assert n_amb <= 1, "%s: %d ambiguous rows: choose another seed" % (c.tag(), n_amb)
        if kind != "bc" and c.B >= 15:
            above, below, inside = lp.branches(c)
            assert above and below and inside, "%s: clipped above / below / unclipped rows %s" % (c.tag(), (above, below, inside))
        if c.B >= 15:
            assert (c.cmds == -1).any() and (c.cmds == c.C).any()
            if kind != "ppo":
                assert any((c.actions[h][c.kindrow[h] == 1] == -1).any() for h in range(2)) and \
                    any((c.actions[h][c.kindrow[h] == 1] == c.Ks[h]).any() for h in range(2))


def test_variants_of_the_imitation_kernel(cases):
    """weights NULL, statistics off and the evaluation form are the same statements on other operands."""
    c = cases["bc"][1]
    ref = lp.run_loss(c, XVE, weights=False)
    lp.check_loss(c, lp.emulate_loss(c, "tree", weights=False), ref, c.tag() + ", no weights")
    got = lp.emulate_loss(c, "tree", grad=False)
    assert (got["dlogits"] == lp.SENT).all() and (got["dvalues"] == lp.SENT).all()
    lp.check_loss(c, got, lp.run_loss(c, XVE, grad=False), c.tag() + ", evaluation form", grad=False)


def test_planted_ties_are_exact(cases, refs):
    """The planted rows carry no comparison the bounds leave open between branches that differ: v == v_old, v_old = 0 and v = clip,
    adv == 0, the max tie outside the clamp (clip 0.125), the ratio on the clamp (clip 0, one bin)."""
    for c, ref in zip(cases["ppo"], refs["ppo"]):
        if c.B < 15:
            continue
        assert not (ref["amb"] & c.planted).any(), c.tag()
    c, ref = cases["ppo"][3], refs["ppo"][3]                     # clip 0.125: v_old = 0, v = 5 clip, R = 3 clip -> 0.5 * 2 (v - R), no error
    i = (c.C + c.cmds[1, 7]) * c.v_ns + 7 * c.ldv
    want = float(c.hp["value_coeff"]) * float(c.hp["inv_b"]) * 0.5 * (0.5 * 2 * (5 * 0.125 - 3 * 0.125))
    assert abs(ref["dvalues"].v[i] - want) < 1e-15 and ref["dvalues"].e[i] <= 2 * lp.U * abs(want)
    c, ref = cases["ppo"][4], refs["ppo"][4]                     # clip 0, K = 1, old_logp = 0: ratio = 1 exactly, on both clamp ends
    assert c.planted[0, 6] and not ref["amb"][0, 6]


# ----------------------------------------------------------------------------- the probe
def _probe(K, scale, floor=True, n=4096, seed=5):
    r = np.random.RandomState(seed + K)
    x = (r.standard_normal((n, K)) * scale).astype(F4)
    a = r.randint(0, K, n)
    v, ov, R, A = (r.standard_normal(n).astype(F4) for _ in range(4))
    lg = lp.front(X64(), x.astype(F8))[0]
    olp = (lg[np.arange(n), a] + 0.3 * r.standard_normal(n)).astype(F4)
    hp = (0.1, 0.5, 1.0, 0.01, 1.0 / n)
    keep = lp.FLOOR
    try:
        if not floor:
            lp.FLOOR = 0.0
        X = XVE(n)
        ref = lp.ppo_row(X, *(X.c(t) for t in (x,)), a, *(X.c(t) for t in (v, ov, R, olp, A)), hp)[0]
    finally:
        lp.FLOOR = keep
    worst, out = 0.0, 0
    for order in ("tree", "seq"):
        got = lp.ppo_row(X32(order), x, a, v, ov, R, olp, A, hp)[0]
        q = np.abs(got.astype(F8) - ref.v)[~X.amb] / ref.e[~X.amb]
        worst, out = max(worst, float(q.max())), max(out, int((q > 1).sum()))
    med = float(np.median(ref.e[ref.v != 0] / np.abs(ref.v[ref.v != 0])))
    return worst, out, med, int(X.amb.sum()), n * K


@pytest.mark.parametrize("K", [3, 33, 64])
def test_probe_of_the_plain_categorical_gradient(K):
    left = 0
    for scale in (1.0, 4.0, 16.0):
        worst, out, med, amb, n = _probe(K, scale)
        print("probe K %d scale %g: honest fp32 at %.3f of the bound, median bound %.2e of the element, %d ambiguous rows of 4096" % (K, scale, worst, med, amb))
        assert out == 0 and worst <= 1.0 and amb <= 4
        w0, out0, _m, _a, _n = _probe(K, scale, floor=False)
        print("      without the 2^-126 floor: %d of %d elements (%.2f %%) leave the bound" % (out0, n, 100.0 * out0 / n))
        left += out0 if scale == 16.0 else 0
        assert scale == 16.0 or out0 == 0
    assert K == 3 or left > 0, "the floor is there for expf's underflow at scale 16"


# ----------------------------------------------------------------------------- the front
@pytest.mark.parametrize("K,ordinal", [(33, False), (64, True), (3, True), (1, False)])
def test_front_emulation_inside(K, ordinal):
    r = np.random.RandomState(K)
    x = lp.raw_rows(r, 48, K, 4.0, ordinal)
    rk = lp.rank_table(K, ordinal)[:K].astype(np.int64) if ordinal else None
    X, lg, pk, H = lp.front_reference(x, rk)
    for order in ("tree", "seq"):
        g = lp.front(X32(order), x, rk)
        rep = lp.Report("front K %d %s %s" % (K, "ordinal" if ordinal else "categorical", order))
        rep.check("lg", g[0], lg)
        rep.check("p", g[1], pk)
        rep.check("H", g[2], H)
        rep.finish()
        cand = lp.candidates(pk)
        assert cand[np.arange(48), np.argmax(g[1], -1)].all()


# ----------------------------------------------------------------------------- mutants
def _fails(c, ref, mut, **kw):
    try:
        with np.errstate(all="ignore"):
            got = lp.emulate_loss(c, "tree", mut=mut, **kw)
        lp.check_loss(c, got, ref, "mutant", quiet=True)
    except AssertionError as e:
        return str(e).splitlines()[1].strip()
    return None


def _old_ppo_inputs(B, scale):
    """The inputs of tests/test_kernels_gpu.py::test_ppo_loss_fwd_bwd."""
    g = torch.Generator().manual_seed(B)
    nS, nT = 33, 3
    logits = torch.zeros(8, B, 64); values = torch.randn(8, B, generator=g)
    logits[:4, :, :nS] = torch.randn(4, B, nS, generator=g) * scale
    logits[4:, :, :nT] = torch.randn(4, B, nT, generator=g) * scale
    actions = torch.stack([torch.randint(0, nS, (B,), generator=g), torch.randint(0, nT, (B,), generator=g)])
    cmds = torch.randint(0, 4, (2, B), generator=g, dtype=torch.int32)
    old_v = torch.randn(2, B, generator=g); rets = torch.randn(2, B, generator=g); adv = torch.randn(2, B, generator=g)
    old_lp = torch.stack([torch.full((B,), -np.log(nS)), torch.full((B,), -np.log(nT))]) + 0.3 * torch.randn(2, B, generator=g)
    hp = dict(clip=0.1, value_coeff=0.1, clip_coeff=1.0, ent_coeff=0.01, inv_b=1.0 / B)
    return lp.LossCase.from_arrays("ppo", logits, values, actions, cmds, rets, (nS, nT), 4, (None, None), hp, old_v, old_lp.float(), adv)


def _old_ord_inputs(case):
    """The inputs of tests/test_ordinal_gpu.py::test_loss_ord_fwd_bwd."""
    from tests import test_ordinal_gpu as og
    B, C, nS, nT, _s = case
    inp, ranks, _ref = og.loss_case(*case)
    hp = dict(clip=og.CLIP, value_coeff=og.VC, clip_coeff=og.CC, ent_coeff=og.EC, inv_b=1.0 / B)
    return lp.LossCase.from_arrays("ppo", inp["logits"], inp["values"], inp["actions"], inp["cmds"], inp["rets"], (nS, nT), C, ranks, hp,
                                   inp["old_v"], inp["old_lp"], inp["adv"])


def _old_bc_inputs(case, scale, weighted, eps):
    """The inputs of tests/test_imitation_gpu.py::test_bc_loss_fwd_bwd."""
    from tests import test_imitation_gpu as ig
    B, C, nS, nT = case
    inp, _ranks = ig.bc_case(B, C, nS, nT, scale, weighted)
    hp = dict(smoothing=eps, bc_coeff=ig.BC, value_coeff=ig.VC, ent_coeff=ig.EC, inv_b=1.0 / B)
    return lp.LossCase.from_arrays("bc", inp["logits"], inp["values"], inp["actions"], inp["cmds"], inp["rets"], (nS, nT), C, (None, None), hp,
                                   weights=inp["w"])


def _old_mix_inputs(case):
    """The inputs of tests/test_demo_mix_gpu.py::test_sums_against_float64 and its gradient tests."""
    from tests import test_demo_mix_gpu as mg
    B, B_ppo, C = case
    inp, _ranks = mg.mix_case(B, B_ppo, C)
    inv_b, inv_bd = mg.scales(B, B_ppo)
    hp = dict(clip=mg.CLIP, value_coeff=mg.VC, clip_coeff=mg.CC, ent_coeff=mg.EC, inv_b=inv_b, smoothing=mg.EPS, demo_coeff=mg.DC,
              demo_value_coeff=mg.DVC, inv_bd=inv_bd)
    return lp.LossCase.from_arrays("mix", inp["logits"], inp["values"], inp["actions"], inp["cmds"], inp["rets"], (mg.NS, mg.NT), C, (None, None),
                                   hp, inp["old_v"], inp["old_lp"], inp["adv"], inp["kind"])


def _old_metric(olds, mut, honest=False):
    """The worst old-metric value of dlogits and dvalues over the old tests' inputs (the bars: 2e-5 and 1e-5)."""
    worst = [0.0, 0.0]
    for c in olds:
        ref = lp.run_loss(c, X64())
        with np.errstate(all="ignore"):
            got = lp.emulate_loss(c, "tree", mut=() if honest else mut)
        with np.errstate(invalid="ignore"):
            for j, k in enumerate(("dlogits", "dvalues")):
                m = lp.old_metric(got[k], ref[k])
                worst[j] = max(worst[j], m if np.isfinite(m) else float("inf"))
    return worst


LOSS_MUTANTS = [
    # name, mutant, kind of the new cases it runs on, the old tests whose inputs give the old metric
    ("entropy gradient without H", {"ent_no_H"}, "ppo", "ppo"),
    ("entropy gradient skipped where p < 1e-6", {"ent_skip_small"}, "ppo", "ppo"),
    ("sigmoid(-x) formed as 1 - s", {"one_minus_s"}, "ppo", "ord"),
    ("ordinal logs without their eps", {"ord_no_eps"}, "ppo", "ord"),
    ("ordinal logs with eps outside the log", {"ord_eps_outside"}, "ppo", "ord"),
    ("the max tie taken wholly from one side", {"tie_one_side"}, "ppo", "ppo"),
    # in_ratio alone is no mutant that any stored output can show: ratio = expf(lp - old_logp) meets 1 +- clip exactly only where it can be
    # planted, on a head with one bin (lp = 0 without error), and there d total / d logit is dlp (1 - p) = 0 whatever dlp is (case
    # "clip 0, K = 1" plants that row all the same: the tie must not turn into an ambiguous row).  The pair is held through in_v
    ("in_ratio and in_v exclusive", {"in_ratio_excl", "in_v_excl"}, "ppo", "ppo"),
    ("in_v exclusive", {"in_v_excl"}, "ppo", "ppo"),
    ("a demonstration row scaled by inv_b", "demo_inv_b", "mix", "mix"),
    ("the weight missing from dvalues", {"w_missing_dvalues"}, "bc", "bc"),
    ("t_off = eps / (K - 1)", {"t_off_km1"}, "bc", "bc"),
    ("columns K .. ldl-1 left unwritten", {"cols_unwritten"}, "ppo", "ppo"),
]
@pytest.fixture(scope="module")
def olds():
    from tests import test_demo_mix_gpu as mg
    from tests import test_imitation_gpu as ig
    from tests import test_ordinal_gpu as og
    return dict(ppo=[_old_ppo_inputs(B, s) for B, s in ((16, 1.0), (64, 4.0), (200, 1.0), (7, 2.0))],
                ord=[_old_ord_inputs(c) for c in og.CASES],
                bc=[_old_bc_inputs(c, s, w, 0.1) for c in ig.CASES for s in (1.0, 4.0) for w in (False, True)],
                mix=[_old_mix_inputs(c) for c in mg.CASES])


def _loss_old_metric(olds, mut, old):
    """(dlogits, dvalues) in the old metric, the worst over the old tests' inputs."""
    if mut != "demo_inv_b":
        return _old_metric(olds[old], mut)
    om = [0.0, 0.0]
    for c in olds[old]:
        om = [max(a, b) for a, b in zip(om, _old_metric([c], {"demo_inv_b": c.hp["inv_b"]}))]
    return om


@pytest.mark.parametrize("name,mut,kind,old", LOSS_MUTANTS, ids=[m[0] for m in LOSS_MUTANTS])
def test_loss_mutants_fail(cases, refs, olds, name, mut, kind, old):
    killed = None
    for c, ref in zip(cases[kind], refs[kind]):
        killed = _fails(c, ref, {"demo_inv_b": c.hp["inv_b"]} if mut == "demo_inv_b" else mut)
        if killed:
            killed = "%s: %s" % (c.tag(), killed)
            break
    om = _loss_old_metric(olds, mut, old)
    print("mutant '%s': old metric on the old inputs dlogits %.2e (bar 2e-5) dvalues %.2e (bar 1e-5): the old bars %s it; new bound: %s"
          % (name, om[0], om[1], "PASS" if om[0] < 2e-5 and om[1] < 1e-5 else "fail", killed))
    assert killed, "mutant '%s' passes the bound at every case" % name


def test_honest_emulation_passes_the_old_bars_too(olds):
    for k, cs in olds.items():
        om = _old_metric(cs, (), honest=True)
        assert om[0] < 2e-5 and om[1] < 1e-5, (k, om)


# ----------------------------------------------------------------------------- clip + Adam
def _adam_chain(case, X, mut=(), steps=3):
    """Three chained steps in the arithmetic of X (the norms from the float64 sum of squares) -> [(p, m, v)] per step."""
    p, m, v = case.p0, case.m0, case.v0
    out = []
    for step in range(1, steps + 1):
        g = case.grads[step - 1]
        n2 = lp.norms2_ref(g, case.seg_off).v
        p, m, v = lp.adam_step(case, X, step, p, g, m, v, n2, mut=mut)
        out.append((p, m, v))
    return out


ADAM_CASES = [dict(seed=71), dict(seed=72, aligned=False), dict(seed=73, warm=True)]


@pytest.mark.parametrize("kw", ADAM_CASES, ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
def test_adam_emulation_inside(kw):
    case = lp.AdamCase(**kw)
    p, m, v = case.p0, case.m0, case.v0
    bites = []
    for step in (1, 2, 3):
        g = case.grads[step - 1]
        n2 = lp.norms2_ref(g, case.seg_off).v
        bites += [math.sqrt(x) > case.max_norm for x, n in zip(n2, case.sizes) if n]
        ref = lp.adam_step(case, XVE, step, p, g, m, v, n2)
        got = lp.adam_step(case, X32(), step, p, g, m, v, n2)
        rep = lp.Report("clip + Adam %s step %d" % (kw, step))
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), got, ref):
            rep.check(name, a, b)
        rep.finish()
        p, m, v = got
    assert any(bites) and not all(bites), "the clip must bite in some segments and not in others"
    assert float(np.abs(case.grads[0][case.grads[0] != 0]).min()) < 1e-9 and float(np.abs(case.grads[0]).max()) > 10


ADAM_MUTANTS = [("Adam eps inside the bias-corrected root", {"eps_inside"}), ("Adam w2 and beta2 exchanged", {"w2_beta2_swapped"}),
                ("clip coefficient on m but not on v", {"clip_m_only"})]


def _old_adam_case():
    """The inputs of tests/test_kernels_gpu.py::test_clip_adam."""
    g = torch.Generator().manual_seed(2)
    sizes = [1000, 257, 4096, 33]
    case = lp.AdamCase(0, sizes=sizes, aligned=False)
    case.p0 = torch.randn(case.n, generator=g).numpy()
    case.m0[:], case.v0[:] = 0, 0
    case.grads = [(torch.randn(case.n, generator=g) * torch.repeat_interleave(torch.tensor([30.0, 0.01, 5.0, 100.0]), torch.tensor(sizes))).numpy()
                  for _ in range(3)]
    return case


def _adam_old_metric(mut):
    """max|params - ref| over the three chained steps of test_clip_adam on its inputs, against its reference (oracle.ppo_ref.chief_step)."""
    from oracle import ppo_ref
    old = _old_adam_case()
    off, k = old.seg_off, len(old.sizes)
    params = {"m%d" % i: {"w": torch.from_numpy(old.p0[off[i]:off[i + 1]].copy())} for i in range(k)}
    adam = {n: {"w": (torch.zeros_like(v["w"]), torch.zeros_like(v["w"]))} for n, v in params.items()}
    got, worst = _adam_chain(old, X32(), mut), 0.0
    for step in (1, 2, 3):
        gr = old.grads[step - 1]
        grads = {"m%d" % i: {"w": torch.from_numpy(gr[off[i]:off[i + 1]].copy())} for i in range(k)}
        ppo_ref.chief_step(params, grads, adam, step, lr=lp.ADAM["lr"], max_grad_norm=old.max_norm)
        want = torch.cat([params["m%d" % i]["w"] for i in range(k)]).numpy()
        worst = max(worst, float(np.abs(got[step - 1][0].astype(F8) - want).max()))
    return worst


@pytest.mark.parametrize("name,mut", ADAM_MUTANTS, ids=[m[0] for m in ADAM_MUTANTS])
def test_adam_mutants_fail(name, mut):
    killed = None
    for kw in ADAM_CASES:
        case = lp.AdamCase(**kw)
        g = case.grads[0]
        n2 = lp.norms2_ref(g, case.seg_off).v
        ref = lp.adam_step(case, XVE, 1, case.p0, g, case.m0, case.v0, n2)
        got = lp.adam_step(case, X32(), 1, case.p0, g, case.m0, case.v0, n2, mut=mut)
        rep = lp.Report("mutant")
        for nm, a, b in zip(("params", "exp_avg", "exp_avg_sq"), got, ref):
            rep.check(nm, a, b)
        if rep.bad:
            killed = "%s: %s" % (kw, rep.bad[0])
            break
    om = _adam_old_metric(mut)
    print("mutant '%s': old metric max|params - ref| %.2e on the old inputs (bar 2e-7): the old bar %s it; new bound: %s"
          % (name, om, "PASS" if om < 2e-7 else "fail", killed))
    assert killed, "mutant '%s' passes the bound" % name


def test_at_least_three_mutants_pass_the_old_bars(olds):
    """At least three of the mutants that the bound rejects are ones the existing bars pass.  By arithmetic the p < 1e-6 skip, the eps-less
    ordinal log and the Adam eps placement were expected; the file confirms the first and names others for the other two (the old ordinal
    inputs at scale 4 saturate units; test_clip_adam's segment scaled by 0.01 holds gradients near 4e-5)."""
    passing = [name for name, mut, _kind, old in LOSS_MUTANTS if (lambda om: om[0] < 2e-5 and om[1] < 1e-5)(_loss_old_metric(olds, mut, old))]
    passing += [name for name, mut in ADAM_MUTANTS if _adam_old_metric(mut) < 2e-7]
    print("mutants that the old bars pass: %s" % passing)
    assert "entropy gradient skipped where p < 1e-6" in passing
    assert len(set(passing) - {"in_ratio and in_v exclusive"}) >= 3                  # (that one is `in_v exclusive` once more)
    assert _adam_old_metric(()) < 2e-7                                                # the honest emulation passes the old Adam bar
