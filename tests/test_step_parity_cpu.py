"""CPU: the helpers of tests/step_parity.py against brute force, and the teeth of the bounds it applies — on fp32 numpy emulations of
the mode-3 product and of the sampling launch, never on a kernel.  The truncation mutants pass the old `rel < 2e-5` bar of
tests/test_kernels_gpu.py and break the element-wise bound: that is the gap tests/test_step_parity_gpu.py closes."""
import numpy as np
import pytest
import torch

from tests import f32_parity as fp
from tests import step_parity as sp

F4, F8 = np.float32, np.float64


# ----------------------------------------------------------------------------- own rows and the untouched mask against brute force
def _descs():
    out = [sp.a1_case(i)[0] for i in range(len(sp.A1_CASES))] + [sp.a2_case(i)[0] for i in range(len(sp.A2_CASES))]
    for i, (P, _seg) in enumerate(sp.A3_CASES):
        out.append(sp.a3_dw(i)[0])
        for bm in (32, 64, 128):
            if P % bm == 0:
                out += [sp.a3_dx(i, bm)[0], sp.a3_dh(i, bm)[0]]
    return out


def _brute_own(d, z):
    """(z, row) by (z, row): the definition in include/cadre_hip.h, one row at a time."""
    beg, cnt = (int(v) for v in d.seg[z // d.seg_div])
    rows = []
    for row in range(d.S * d.period):
        b = row % d.period
        if d.mode == 1:
            t0 = b - b % d.bm
            own = cnt > 0 and not (t0 + d.bm <= beg or t0 >= beg + cnt)
        else:
            own = beg <= b < beg + cnt
        if own:
            rows.append(row)
    return np.asarray(rows, np.int64)


def test_own_rows_and_untouched_mask_against_brute_force():
    descs = _descs()
    assert {d.mode for d in descs} == {1, 2, 3}
    for d in descs:
        slots = 1 + max(sp.slot(z, d.c_z) for z in range(d.Z))
        mask = sp.untouched(d, slots, d.M + 3)
        want = np.ones_like(mask)
        for z in range(d.Z):
            rows = _brute_own(d, z)
            assert np.array_equal(sp.own_rows(d, z), rows), (d.what, z)
            for row in (range(d.M) if d.mode == 2 else rows):
                for col in range(d.N):
                    want[sp.slot(z, d.c_z), row, col] = False
        assert np.array_equal(mask, want), d.what
        assert mask[:, d.M:].all() and mask[:, :, d.N:].all()
    # mode 3's compact order (mc -> (mc / cnt) period + beg + mc % cnt) is the ascending order own_rows returns
    d = sp.a1_case(1)[0]
    for z in range(d.Z):
        beg, cnt = d.run(z)
        comp = [(mc // cnt) * d.period + beg + mc % cnt for mc in range(d.S * cnt)]
        assert comp == sp.own_rows(d, z).tolist()


def test_case_tables_hold_what_the_issue_lists():
    runs = [tuple(r) for c in sp.A1_CASES for t in c[4:] for r in t]
    periods = {tuple(r): c[3] for c in sp.A1_CASES for t in c[4:] for r in t}
    assert any(c == 0 for _b, c in runs) and any(c == 1 for _b, c in runs)
    assert any(b == 0 and c == periods[(b, c)] for b, c in runs)
    assert any(b % 32 and (b + c) % 32 and c > 32 for b, c in runs)
    assert all(c[4] != c[5] for c in sp.A1_CASES)
    assert {c[3] for c in sp.A1_CASES} == {64, 96, 100} and {c[2] for c in sp.A1_CASES} == {1, 3}
    assert {(c[0], c[1]) for c in sp.A1_CASES} == {(2120, 2176), (96, 96)}
    assert {c[0] for c in sp.A2_CASES} == {1, 5, 17, 32} and {c[1] for c in sp.A2_CASES} == {1, 2}
    kinds = set()
    for i in range(len(sp.A2_CASES)):
        d, _ops, pos = sp.a2_case(i)
        cnt = d.seg[:sp.C_CMDS, 1]
        kinds |= {"one"} if (cnt == d.period).any() else set()
        kinds |= {"empty"} if (cnt == 0).any() else set()
        kinds |= {"permuted"} if not np.array_equal(pos, np.arange(len(pos))) else set()
        assert int(cnt.sum()) == d.period
    assert kinds == {"one", "empty", "permuted"}


# ----------------------------------------------------------------------------- the ring model against a list of frames
def test_ring_model_against_a_list_of_frames():
    r = np.random.RandomState(5)
    N, S, DPx, n_ring, env_str, ldx, ldf, ldfr = 5, 3, 530, 7, 3 * 512 + 24, 536, 531, 520
    model = sp.RingModel(n_ring, S, env_str, -3.0)
    frames = [None] * N                                              # per environment: the list of its last S latents
    pos = np.array([2, 0, 4, 1, 3], np.int32)
    for step in range(4):
        modes = [0] * N if step == 0 else [int(v) for v in r.randint(0, 2, N)]
        first, nf = sp.window_firsts(modes, S)
        fresh = r.standard_normal((nf + 2, ldfr)).astype(F4)
        meas = sp.awkward_measurements(r, N, S)
        X, feat = np.full((S, N, ldx), 9.0, F4), np.full((N, S, ldf), 9.0, F4)
        model.step(fresh, modes, first, meas, pos, DPx, X, feat)
        k = 0
        for e in range(N):
            if modes[e]:
                frames[e] = frames[e][1:] + [fresh[k, :512]]
                k += 1
            else:
                frames[e] = [fresh[k + s, :512] for s in range(S)]
                k += S
            assert first[e] == k - (1 if modes[e] else S)
            for s in range(S):
                want = np.concatenate([frames[e][s], [F4(meas[e, s, j % 3]) for j in range(18)]]).astype(F4)
                assert np.array_equal(X[s, pos[e], :530], want) and np.array_equal(feat[e, s, :530], want)
                assert np.array_equal(model.ring[e, s * 512:(s + 1) * 512], frames[e][s])
        assert k == nf and (X[:, :, 530:] == 9.0).all() and (feat[:, :, 530:] == 9.0).all()
        assert (model.ring[N:] == -3.0).all() and (model.ring[:, S * 512:] == -3.0).all()
    # the measurements: to nearest, not truncated
    m = sp.awkward_measurements(r, 2, 2)
    assert F4(m[0, 0, 0]) != np.nextafter(F4(m[0, 0, 0]), F4(0)) and abs(F8(F4(m[0, 0, 0]))) > abs(m[0, 0, 0])


# ----------------------------------------------------------------------------- teeth of the product bound on the mode-3 emulation
MUTANTS = ("trunc16", "trunc19", "bias_next", "no_period", "tail_row", "drop")


@pytest.mark.parametrize("which", ["A1", "A2"])
def test_mode3_emulation_passes_and_every_mutant_breaks(which):
    """The 19-bit mutant sits AT the bound, not far outside it: its worst element over the six operand draws 0 .. 5 of the act-form case is
    6.461 / 6.717 / 7.460 / 7.853 / 6.307 / 7.575 units against c_bar = 7.472 / 7.334 / 6.743 / 6.671 / 6.025 / 6.166 (the doubled worst
    error of the sequential chain, itself a maximum over 6528 outputs) — outside in four of six.  The act-form case here is draw 3, picked
    from these CPU figures alone; the update-form case (56736 outputs: 8.320 against 7.323) is its first draw."""
    if which == "A1":
        d, ops = sp.a1_case(4)                                       # 96 / 96, S = 3, B = 100
    else:
        d, ops, _pos = sp.a2_case(9, draw=3)                         # 96 / 96, S = 2, 17 environments; the draw: see the docstring
    assert d.S > 1
    ref = sp.reference(d, ops)
    cb = max(c for _z, e, c, _cap in ref if e is not None)
    cap = max(c for _z, _e, _cb, c in ref)
    assert 0 < cb <= cap == fp.DIRECT_CAP(sp.DP)
    for order in ("seq", "chunk"):
        got = sp.emulate3(d, ops, order)
        st = sp.check_case(d, ref, got, torch.full_like(got, sp.FILL), "%s emulation %s" % (d.what, order))
        assert st[0] <= st[1] <= st[2]
    for mut in MUTANTS:
        got = sp.emulate3(d, ops, "seq", mut)
        bad, old, st = sp.measure_case(d, ref, got)
        print("%s mutant %-9s: excess %8.3f units (c_bar %.3f), old metric %.3g" % (d.what, mut, st["excess"], st["c_bar"], old))
        assert bad, "%s: mutant %s passes the bound" % (d.what, mut)
        if mut.startswith("trunc"):
            assert old < 2e-5, "%s: mutant %s no longer passes the old bar (%.3g)" % (d.what, mut, old)
        with pytest.raises(AssertionError):
            sp.check_case(d, ref, got, torch.full_like(got, sp.FILL), "mutant " + mut)


def test_untouched_elements_are_checked():
    d, ops = sp.a1_case(3)
    ref = sp.reference(d, ops)
    got = sp.emulate3(d, ops)
    fill = torch.full_like(got, sp.FILL)
    sp.check_case(d, ref, got, fill, d.what)
    for where in ((0, 40, 0), (3, 0, 0), (7, 63, 95)):                # a foreign row of net 0, a row of an empty run, the last own element's neighbour
        g = got.clone()
        z, row, col = where
        if not sp.untouched(d, d.Z, d.M)[where]:
            row = int(np.setdiff1d(np.arange(d.M), sp.own_rows(d, z))[0])
        g[z, row, col] = float(np.nextafter(F4(sp.FILL), F4(8)))
        with pytest.raises(AssertionError, match="outside the rows"):
            sp.check_case(d, ref, g, fill, d.what)


def test_mode2_empty_net_and_mode1_reference():
    d, ops = sp.a3_dw(0)
    ref = sp.reference(d, ops)
    empty = [z for z in range(d.Z) if d.run(z)[1] == 0]
    assert empty
    for z, e, cb, cap in ref:
        assert cap == fp.DIRECT_CAP(sp.A3_S * d.period)
        if z in empty:
            assert cb is None and not e["mag"].any() and not e["y"].any()
        else:
            want = ops["A"][z].double().t() @ ops["B"][z // 2].double()
            assert torch.equal(e["y"], want)
    d, ops = sp.a3_dx(1, 32)
    for z, e, cb, cap in sp.reference(d, ops):
        if e is not None:
            assert torch.equal(e["y"], (ops["A"][z].double() @ ops["B"][z].double())[torch.from_numpy(e["rows"])]) and cap == fp.DIRECT_CAP(sp.A3_NY)


def test_colsum_and_relu_references():
    r = np.random.RandomState(2)
    X = torch.from_numpy(r.standard_normal((4, 70, 130)).astype(F4))
    prev = torch.from_numpy(r.standard_normal((4, 130)).astype(F4))
    for acc in (0, 1):
        y, mag, cb, cap = sp.colsum_reference(X, prev, acc)
        assert torch.allclose(y.view(4, 130), X.double().sum(1) + (prev.double() if acc else 0)) and cap == fp.DIRECT_CAP(70) and 0 < cb <= cap
        assert torch.allclose(mag.view(4, 130), X.double().abs().sum(1) + (prev.double().abs() if acc else 0))
    y, mag, cb, cap = sp.colsum_reference(X[:, :1, :3], prev[:, :3], 1)          # one row, accumulating: a single addition
    assert 0 < cb <= 2.0 and cap == fp.DIRECT_CAP(1)
    sub = np.float32(1e-45)
    act = np.array([1.0, 0.0, -0.0, sub, -1.0, 2.0], F4)
    dy = np.array([-0.0, 1.0, 2.0, 3.0, 4.0, sub], F4)
    want = sp.relu_bwd_reference(act, dy)
    assert want.view(np.uint32).tolist() == [0x80000000, 0, 0, F4(3.0).view(np.uint32), 0, 1]


# ----------------------------------------------------------------------------- the sampling launches: seeds, emulation, mutants
def test_sampling_reference_meets_the_ambiguity_cap_at_every_seed():
    n = 0
    for kw in sp.sample_cases():
        c = sp.SampleCase(**kw)
        amb = c.ambiguous()
        assert amb <= 1, "choose another seed: %r has %d ambiguous pairs" % (kw, amb)
        n += 1
    assert n >= 24


@pytest.mark.parametrize("order", ["tree", "seq"])
def test_sampling_emulation_inside(order):
    for kw in sp.sample_cases()[::5]:
        c = sp.SampleCase(**kw)
        act, logp, val = c.emulate(order)
        _w, amb = sp.check_sample(c, act, logp, val, "emulation %s %r" % (order, kw), quiet=True)
        assert amb <= 1


def _breaks(c, *a, **k):
    with np.errstate(invalid="ignore"):                              # (a mutant's 0 * -inf in the entropy nobody reads)
        act, logp, val = c.emulate(*a, **k)
    try:
        sp.check_sample(c, act, logp, val, "mutant", quiet=True)
    except AssertionError:
        return True
    return False


def test_sampling_mutants_break():
    cmds = sp.A2_CMDS[17]
    c = sp.SampleCase(seed=11, cmds=[0] * 32, C=1, Ks=(33, 64), ordinal=(True, True))      # one net per head: every row family is read
    assert not _breaks(c)
    for mut in ("one_minus_s", "ord_no_eps", "ord_eps_outside"):     # loss_parity's hooks on the front of an ordinal head
        assert _breaks(c, mut=(mut,)), mut
    for ordinal in ((False, False), (True, True)):
        c = sp.SampleCase(seed=12, cmds=cmds, C=4, Ks=(33, 33), ordinal=ordinal, Mg=2, m0=1, M=4)
        assert not np.array_equal(c.pos, np.arange(c.N))
        assert not _breaks(c)
        assert _breaks(c, row_of=lambda e: e), "row e for row pos[e]"
        assert _breaks(c, tower_of=lambda h, j, e: c.tower(0, j, e)), "head 0's tower for head 1"
