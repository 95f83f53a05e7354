"""GPU: the row-segment modes of cadre_gemm_f32, the three glue launches of the unfused MLP backward and the act launch chain through
the C ABI, EVERY owned element, at the bounds of tests/step_parity.py — the products under f32_parity's |got - y64| <= c_bar 2^-24 mag
(c_bar from the CPU chain of the case's own products, asserted under DIRECT_CAP(K)), the sampling launches under loss_parity's running
first-order bound, the copies and masks bit for bit.  Everything a launch must not write (foreign rows, ldc padding, the tiles of empty
runs, agents outside the group, a margin behind every buffer) keeps its fill bit for bit.  Every product case prints one line:
excess (units) <= c_bar <= cap; every sampling launch one line: worst err / bound, ambiguous pairs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests import step_parity as sp
from tests import update_parity as up
from tests.step_parity import DP, F4, FILL, MARGIN

pytestmark = pytest.mark.gpu
SENT = float(lp.SENT)


def dev(x):
    return torch.as_tensor(x).cuda()


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32 if t.element_size() == 4 else np.uint64)


def cbuf(*shape, fill=FILL):
    """A C buffer of `shape` with MARGIN floats behind it, all `fill` -> (flat buffer, the view, the fill on the host)."""
    n = int(np.prod(shape))
    buf = torch.full((n + MARGIN,), fill, device="cuda")
    return buf, buf[:n].view(*shape), torch.full(shape, fill)


def margin_kept(buf, n, what, fill=FILL):
    tail = buf[n:].cpu()
    assert bool((tail == fill).all()), "%s: the margin behind the buffer was written" % what


def seg32(d):
    return dev(np.ascontiguousarray(d.seg, dtype=np.int32))


def picked_tile(hip, M, N, K, a_mode, b_mode, batch, tile, seg_mode, period, seg_div):
    """cadre_gemm_pick_tile for the descriptor's shape (host logic, no launch)."""
    g = hip.GemmDesc()
    g.M, g.N, g.K, g.a_mode, g.b_mode, g.batch, g.tile, g.split_k = M, N, K, a_mode, b_mode, batch, tile, 1
    g.seg_mode, g.seg_period, g.seg_div = seg_mode, period, seg_div
    t = hip.lib().cadre_gemm_pick_tile(C.byref(g))
    assert t in sp.TILE_BM, "tile %d has no M-tile size in step_parity.TILE_BM" % t
    return t


def summary(group, stats):
    """One line per test: the group's worst excess / c_bar ("fp32 parity", quotes these)."""
    worst = max(stats, key=lambda s: s[0] / s[1])
    print("step-parity %s: worst excess / c_bar = %.3f / %.3f = %.3f (cap %d)" % (group, worst[0], worst[1], worst[0] / worst[1], worst[2]))


# ----------------------------------------------------------------------------- A1 / A2: seg_mode 3
def _mode3(hip, d, ops, x_div, tiles, group):
    ref = sp.reference(d, ops)
    S, B, N, ldc, Z = d.S, d.period, d.N, d.ldc, d.Z
    X, W, b, seg = dev(ops["A"]), dev(ops["B"]), dev(ops["bias"]), seg32(d)

    def launch(G, tile):                                          # learner.py:944-947
        hip.gemm(X, W, G, S * B, N, DP, DP, DP, ldc, shift=b, batch=Z, a_z=(x_div, 0, S * B * DP), b_z=(1, 0, N * DP),
                 c_z=(1, 0, S * B * ldc), s_z=(1, 0, N), seg=(3, seg, B, 1), tile=tile)
    stats = []
    for tile in tiles:
        buf, G, fill = cbuf(Z, S * B, ldc)
        launch(G, tile)
        torch.cuda.synchronize()
        what = "%s tile %d" % (d.what, tile)
        margin_kept(buf, G.numel(), what)
        stats.append(sp.check_case(d, ref, G.cpu(), fill, what))
    # tile 11: the skinny kernel (A/B build) does not take compact rows, the default build has no tile 11: refused by return value either way
    buf, G, fill = cbuf(Z, S * B, ldc)
    with pytest.raises(hip.CadreHipError):
        launch(G, 11)
    torch.cuda.synchronize()
    assert bool((buf.cpu() == FILL).all()), "%s: the refused tile 11 wrote" % d.what
    summary(group, stats)


@pytest.mark.parametrize("i", range(len(sp.A1_CASES)), ids=lambda i: "N%d-S%d-B%d" % (sp.A1_CASES[i][0], sp.A1_CASES[i][2], sp.A1_CASES[i][3]))
def test_mode3_update_form(hip, i):
    """A1: the LSTM input projection as the update launches it (learner.py:944-947, x_div = C), tiles 0, 3, 8, 9."""
    d, ops = sp.a1_case(i)
    _mode3(hip, d, ops, sp.C_CMDS, sp.A1_TILES, "A1")


@pytest.mark.parametrize("i", range(len(sp.A2_CASES)), ids=lambda i: "envs%d-S%d-%s-N%d" % (sp.A2_CASES[i][0], sp.A2_CASES[i][1], sp.A2_CASES[i][2], sp.A2_CASES[i][3]))
def test_mode3_act_form(hip, i):
    """A2: the same launch as act_batch issues it (agent.py:400-423): period = the number of environments, x_div = 2C, tiles 0, 3, 9."""
    d, ops, _pos = sp.a2_case(i)
    _mode3(hip, d, ops, 2 * sp.C_CMDS, sp.A2_TILES, "A2")


# ----------------------------------------------------------------------------- A3: seg_mode 2 and 1
@pytest.mark.parametrize("i", range(len(sp.A3_CASES)), ids=lambda i: "P%d" % sp.A3_CASES[i][0])
def test_mode2_dw(hip, i):
    """dW = dY^T X (learner.py:1193-1194): k-tiles outside the run are not multiplied, an empty net gives exact zeros."""
    d, ops = sp.a3_dw(i)
    ref = sp.reference(d, ops)
    P, SP, ny, nx, nb = d.period, d.S * d.period, sp.A3_NY, sp.A3_NX, 2 * sp.A3_Z
    dY, X, seg = dev(ops["A"]), dev(ops["B"]), seg32(d)
    stats = []
    for tile in sp.A3_TILES:
        buf, dW, fill = cbuf(nb, ny, nx, fill=3.0)
        hip.gemm(dY, X, dW, ny, nx, SP, ny, nx, nx, a_mode=1, b_mode=1, batch=nb, a_z=(1, 0, SP * ny), b_z=(2, 0, SP * nx),
                 c_z=(1, 0, ny * nx), seg=(2, seg, P, 2), tile=tile)
        torch.cuda.synchronize()
        what = "%s tile %d" % (d.what, tile)
        margin_kept(buf, dW.numel(), what, 3.0)
        got = dW.cpu()
        for z in range(nb):
            if d.run(z)[1] == 0:
                assert not bits(got[z]).any(), "%s: the empty net %d is not all +0" % (what, z)
        stats.append(sp.check_case(d, ref, got, fill, what))
    summary("A3 dW", stats)


@pytest.mark.parametrize("i", range(len(sp.A3_CASES)), ids=lambda i: "P%d" % sp.A3_CASES[i][0])
def test_mode1_dx(hip, i):
    """dX = dY W (learner.py:1197-1198): the M tiles that meet the run are full products, every other tile keeps its fill."""
    P = sp.A3_CASES[i][0]
    SP, ny, nx, nb = sp.A3_S * P, sp.A3_NY, sp.A3_NX, 2 * sp.A3_Z
    refs, stats = {}, []
    for tile in sp.A3_TILES:
        bm = sp.tile_rows(picked_tile(hip, SP, nx, ny, 0, 1, nb, tile, 1, P, 2), 1, P)
        d, ops = sp.a3_dx(i, bm)
        if bm not in refs:
            refs[bm] = sp.reference(d, ops)
        dY, W, seg = dev(ops["A"]), dev(ops["B"]), seg32(d)
        buf, dX, fill = cbuf(nb, SP, nx)
        hip.gemm(dY, W, dX, SP, nx, ny, ny, nx, nx, b_mode=1, batch=nb, a_z=(1, 0, SP * ny), b_z=(1, 0, ny * nx), c_z=(1, 0, SP * nx),
                 seg=(1, seg, P, 2), tile=tile)
        torch.cuda.synchronize()
        what = "%s tile %d" % (d.what, tile)
        margin_kept(buf, dX.numel(), what)
        stats.append(sp.check_case(d, refs[bm], dX.cpu(), fill, what))
    summary("A3 dX", stats)


@pytest.mark.parametrize("i", range(len(sp.A3_CASES)), ids=lambda i: "P%d" % sp.A3_CASES[i][0])
def test_mode1_two_towers_into_dh(hip, i):
    """dH = dA1_actor W1_actor + dA1_critic W1_critic (learner.py:1214-1217): two launches, the second with resid = C.  The second launch's
    reference takes the first launch's device result as the residual operand; mag includes |resid|."""
    P = sp.A3_CASES[i][0]
    SP, ny, nx, Z = sp.A3_S * P, sp.A3_NY, sp.A3_NX, sp.A3_Z
    stats = []
    for tile in sp.A3_TILES:
        bm = sp.tile_rows(picked_tile(hip, SP, ny, nx, 0, 1, Z, tile, 1, P, 1), 1, P)
        d, ops = sp.a3_dh(i, bm)
        A, W, seg = dev(ops["A"]), dev(ops["B"]), seg32(d)
        buf, dH, before = cbuf(Z, SP, ny)
        for tower in (0, 1):
            hip.gemm(A.view(-1)[tower * SP * nx:], W.view(-1)[tower * nx * ny:], dH, SP, ny, nx, nx, ny, ny, b_mode=1, batch=Z,
                     a_z=(1, 0, 2 * SP * nx), b_z=(1, 0, 2 * nx * ny), c_z=(1, 0, SP * ny),
                     resid=dH if tower else None, ldr=ny, r_z=(1, 0, SP * ny), seg=(1, seg, P, 1), tile=tile)
            torch.cuda.synchronize()
            what = "%s tile %d launch %d" % (d.what, tile, tower)
            margin_kept(buf, dH.numel(), what)
            got = dH.cpu()
            o = dict(A=ops["A"][:, tower], B=ops["B"][:, tower], resid=before if tower else None)
            stats.append(sp.check_case(d, sp.reference(d, o), got, before, what))
            before = got.clone()
    summary("A3 dH", stats)


# ----------------------------------------------------------------------------- A4: the glue launches
@pytest.mark.parametrize("M", [1, 3, 24, 70])
def test_colsum(hip, M):
    """cadre_colsum (learner.py:1195) as the product with a column of ones; accumulating: the previous content is the residual."""
    L, batch = hip.lib(), 16
    stats = []
    for N in (3, 128, 130):
        r = np.random.RandomState(10 * M + N)
        ldx, o_str = N + 2, N + 7
        x_str = M * ldx + 5
        X = torch.from_numpy(r.standard_normal((batch, x_str)).astype(F4))
        prev = torch.from_numpy(r.standard_normal((batch, o_str)).astype(F4))
        Xd = dev(X)
        for acc in (0, 1):
            buf = torch.cat([dev(prev).view(-1), torch.full((MARGIN,), FILL, device="cuda")])
            hip.check(L.cadre_colsum(Xd.data_ptr(), ldx, x_str, buf.data_ptr(), o_str, M, N, batch, acc, hip.stream()), "cadre_colsum")
            torch.cuda.synchronize()
            what = "cadre_colsum M %d N %d accumulate %d" % (M, N, acc)
            margin_kept(buf, batch * o_str, what)
            got = buf[:batch * o_str].view(batch, o_str).cpu()
            assert np.array_equal(bits(got[:, N:]), bits(prev[:, N:])), "%s: columns behind N were written" % what
            if M == 1 and not acc:                                 # one product with 1.0 and no addition: there is no rounding to bound
                assert np.array_equal(bits(got[:, :N]), bits(X[:, :N])), what + ": a one-row sum is not the row itself"
                continue
            case = up.Case(what)
            Xv = torch.stack([X[z, :M * ldx].view(M, ldx)[:, :N] for z in range(batch)])
            y, mag, cb, cap = sp.colsum_reference(Xv, prev[:, :N], acc, what)
            case.add_units("out", got[:, :N].reshape(1, batch * N), y, mag, cb, cap)
            stats.append(case.finish()["out"])
    summary("A4 colsum", stats)


def test_relu_bwd(hip):
    """cadre_relu_bwd (learner.py:1209, 1211), exact: kept elements keep their bits, the others are +0; with and without the command mask."""
    L = hip.lib()
    r = np.random.RandomState(3)
    Cn, B, hid = 4, 24, 128
    nb = 2 * 2 * Cn
    n = nb * B * hid
    sub = F4(1e-45)                                               # the smallest positive subnormal
    act = r.standard_normal(n).astype(F4)
    act[::7], act[1::11], act[2::13], act[3::17] = F4(0.0), F4(-0.0), sub, -sub
    dy = r.standard_normal(n).astype(F4)
    dy[::5], dy[1::19] = F4(-0.0), sub
    cmds = r.randint(0, Cn, (2, B)).astype(np.int32)
    act_d, cmd_d = dev(act), dev(cmds)
    for commands, count in ((None, n), (cmds, n), (None, n - 5)):
        buf = torch.cat([dev(dy), torch.full((MARGIN,), FILL, device="cuda")])
        hip.check(L.cadre_relu_bwd(act_d.data_ptr(), buf.data_ptr(), count, None if commands is None else cmd_d.data_ptr(), B, hid, Cn,
                                   hip.stream()), "cadre_relu_bwd")
        torch.cuda.synchronize()
        want = np.concatenate([sp.relu_bwd_reference(act[:count], dy[:count], commands, B, hid, Cn), dy[count:], np.full(MARGIN, FILL, F4)])
        bad = bits(buf) != want.view(np.uint32)
        print("cadre_relu_bwd commands %s n %d: %d elements, %d not bit-identical" % (commands is not None, count, want.size, int(bad.sum())))
        assert not bad.any(), "first at %d" % int(np.argmax(bad))
        kept = want[:count].view(np.uint32) != 0
        assert kept.any() and (~kept).any() and (act[:count][kept] == sub).any()


@pytest.mark.parametrize("x_div", [1, 4, 8])
def test_lstm_init(hip, x_div):
    """cadre_lstm_init (learner.py:941-942), exact: slot 0 of every net <- h0 / c0 of its head block, the gaps between the slots untouched,
    dC exact zeros or NULL."""
    L, Z = hip.lib(), 8
    r = np.random.RandomState(x_div)
    n_per = 5 * DP
    z_str = 3 * n_per + 8
    blocks = Z // x_div
    h0, c0 = (r.standard_normal((blocks, n_per)).astype(F4) for _ in range(2))
    h0[0, :4] = [0.0, -0.0, 1e-45, -1e-45]
    h0d, c0d = dev(h0), dev(c0)
    for with_dc in (False, True):
        Hb, Hs, _ = cbuf(Z, z_str)
        Cb, Cs, _ = cbuf(Z, z_str, fill=-3.0)
        Db, dC, _ = cbuf(Z, n_per, fill=5.0)
        hip.check(L.cadre_lstm_init(h0d.data_ptr(), c0d.data_ptr(), Hs.data_ptr(), Cs.data_ptr(), dC.data_ptr() if with_dc else None,
                                    n_per, z_str, x_div, Z, hip.stream()), "cadre_lstm_init")
        torch.cuda.synchronize()
        for buf, src, fill in ((Hb, h0, FILL), (Cb, c0, -3.0)):
            want = np.full((Z, z_str), fill, F4)
            for z in range(Z):
                want[z, :n_per] = src[z // x_div]
            want = np.concatenate([want.reshape(-1), np.full(MARGIN, fill, F4)])
            assert np.array_equal(bits(buf), want.view(np.uint32)), "cadre_lstm_init x_div %d: state slots differ" % x_div
        want = np.concatenate([np.zeros(Z * n_per, F4) if with_dc else np.full(Z * n_per, 5.0, F4), np.full(MARGIN, 5.0, F4)])
        assert np.array_equal(bits(Db), want.view(np.uint32)), "cadre_lstm_init x_div %d dC %s" % (x_div, with_dc)
    print("cadre_lstm_init x_div %d: %d copied elements per buffer bit-identical, gaps and margins untouched" % (x_div, Z * n_per))


# ----------------------------------------------------------------------------- B1: cadre_act_windows
@pytest.mark.parametrize("N", [1, 5, 17])
@pytest.mark.parametrize("S", [1, 2, 8])
def test_act_windows(hip, N, S):
    """cadre_act_windows against step_parity.RingModel, bit for bit, three successive steps on one ring."""
    L = hip.lib()
    for DPx in (530, 544):
        r = np.random.RandomState(100 * N + 10 * S + DPx)
        n_ring, env_str, ldfr, ldx, ldf = N + 2, S * 512 + 24, 520, DPx + 8, DPx + 3
        pos = np.roll(np.arange(N, dtype=np.int32), 2)[::-1].copy() if N > 1 else np.zeros(1, np.int32)
        assert N == 1 or not np.array_equal(pos, np.arange(N))
        model = sp.RingModel(n_ring, S, env_str, -3.0)
        ring_b, ring, _ = cbuf(n_ring, env_str, fill=-3.0)
        pos_d = dev(pos)
        for step in range(3):
            modes = [(e + step) % 2 for e in range(N)] if N > 1 else [step % 2]      # shifts and resets mixed in every step
            first, nf = sp.window_firsts(modes, S)
            fresh = r.standard_normal((nf, ldfr)).astype(F4)
            meas = sp.awkward_measurements(r, N, S)
            fr_d, mode_d, first_d, meas_d = dev(fresh), dev(np.asarray(modes, np.int32)), dev(first), dev(meas)
            ring_before = ring_b.clone()
            outs = []
            for with_feat in (True, False):
                rb = ring_b if with_feat else ring_before
                Xb, X, _ = cbuf(S, N, ldx, fill=9.0)
                Fb, feat, _ = cbuf(N, S, ldf, fill=9.0)
                hip.check(L.cadre_act_windows(rb.data_ptr(), env_str, n_ring, fr_d.data_ptr(), ldfr, nf, mode_d.data_ptr(), first_d.data_ptr(),
                                              meas_d.data_ptr(), pos_d.data_ptr(), N, S, X.data_ptr(), ldx, DPx,
                                              feat.data_ptr() if with_feat else None, ldf, hip.stream()), "cadre_act_windows")
                torch.cuda.synchronize()
                outs.append((bits(Xb), bits(Fb), bits(rb)))
            what = "cadre_act_windows N %d S %d DP %d step %d" % (N, S, DPx, step)
            wX, wF = np.full((S, N, ldx), 9.0, F4), np.full((N, S, ldf), 9.0, F4)
            model.step(fresh, modes, first, meas, pos, DPx, wX, wF)
            pad = lambda a, fill: np.concatenate([a.reshape(-1), np.full(MARGIN, fill, F4)]).view(np.uint32)
            gX, gF, gR = outs[0]
            assert np.array_equal(gX, pad(wX, 9.0)), what + ": X (rows, the columns behind DP, the margin)"
            assert np.array_equal(gF, pad(wF, 9.0)), what + ": feat"
            assert np.array_equal(gR, pad(model.ring, -3.0)), what + ": the ring (slots >= N and the margin keep their fill)"
            assert np.array_equal(outs[1][0], gX) and np.array_equal(outs[1][2], gR), what + ": feat = NULL changes X or the ring"
            assert np.array_equal(outs[1][1], pad(np.full((N, S, ldf), 9.0, F4), 9.0)), what + ": feat = NULL wrote feat"
            assert np.array_equal(bits(fr_d), fresh.view(np.uint32)), what + ": fresh was written"
            # the issue's columns, spelt out on the device result
            Xg = gX[:S * N * ldx].view(F4).reshape(S, N, ldx)
            for e in range(N):
                m32 = np.tile(meas[e].astype(F4), (1, 6))
                assert np.array_equal(Xg[:, pos[e], 512:530].view(np.uint32), m32.view(np.uint32)), what + ": measurements not rounded to nearest"
                assert not Xg[:, pos[e], 530:DPx].view(np.uint32).any(), what + ": columns 530 .. DP-1 are not +0"
        print("cadre_act_windows N %d S %d DP %d: 3 steps, X / feat / ring bit-identical to the model" % (N, S, DPx))


# ----------------------------------------------------------------------------- B2: cadre_sample_rows / _ord / _ens
def _sample(hip, c, entry, table=None, bad=()):
    """One launch -> (act int64, logp, val fp32) [N][M][2] on the host, with 8 guard elements behind each checked for the fill."""
    L, N, M = hip.lib(), c.N, c.M
    pos, cmd = c.pos.astype(np.int32).copy(), c.cmds.copy()
    for e, what, v in bad:
        (pos if what == "pos" else cmd)[e] = v
    O3, pos_d, cmd_d = dev(c.O3), dev(pos), dev(cmd)
    q_d = None if c.greedy else dev(c.q)
    n = N * M * 2
    act = torch.full((n + 8,), -5, dtype=torch.int64, device="cuda")
    logp, val = torch.full((n + 8,), SENT, device="cuda"), torch.full((n + 8,), SENT, device="cuda")
    head = [O3.data_ptr(), c.ldo, c.z_str, pos_d.data_ptr(), cmd_d.data_ptr(), N, c.C]
    tail = [c.Ks[0], c.Ks[1], act.data_ptr(), logp.data_ptr(), val.data_ptr()]
    tb = None if table is None else dev(table)
    if entry == "cadre_sample_rows":
        rc = L.cadre_sample_rows(*head, q_d.data_ptr(), *tail, hip.stream())
    elif entry == "cadre_sample_rows_ord":
        rc = L.cadre_sample_rows_ord(*head, q_d.data_ptr(), *tail, tb.data_ptr(), hip.stream())
    else:
        rc = L.cadre_sample_rows_ens(*head, c.Mg, c.m0, M, None if q_d is None else q_d.data_ptr(), *tail, None if tb is None else tb.data_ptr(),
                                     hip.stream())
    hip.check(rc, entry)
    torch.cuda.synchronize()
    a, lg, v = act.cpu().numpy(), logp.cpu().numpy(), val.cpu().numpy()
    assert (a[n:] == -5).all() and (lg[n:] == lp.SENT).all() and (v[n:] == lp.SENT).all(), "%s wrote behind its outputs" % entry
    return a[:n].reshape(N, M, 2), lg[:n].reshape(N, M, 2), v[:n].reshape(N, M, 2)


def _check_group(c, out, what, keep_env=None):
    """The group's agents under the bound; every other agent, and every environment not in keep_env, keeps the fill."""
    a, lg, v = out
    g = slice(c.m0, c.m0 + c.Mg)
    outside = np.ones(c.M, bool)
    outside[g] = False
    assert (a[:, outside] == -5).all() and (lg[:, outside] == lp.SENT).all() and (v[:, outside] == lp.SENT).all(), what + ": an agent outside the group was written"
    if keep_env is not None:
        skip = ~np.asarray(keep_env)
        assert (a[skip] == -5).all() and (lg[skip] == lp.SENT).all() and (v[skip] == lp.SENT).all(), what + ": a skipped environment was written"
    worst, amb = sp.check_sample(c, a[:, g], lg[:, g], v[:, g], what, keep_env)
    assert amb <= 1, "%s: %d ambiguous pairs" % (what, amb)
    return worst


@pytest.mark.parametrize("N", sp.SAMPLE_N)
@pytest.mark.parametrize("Cn", sp.SAMPLE_C)
def test_sample_rows(hip, N, Cn):
    """cadre_sample_rows, _ord and _ens statement for statement under loss_parity.front_reference (the test_front block of cadre_sample)."""
    worst = 0.0
    for kw in sp.sample_cases(N, Cn):
        c = sp.SampleCase(**kw)
        tag = "N %d C %d K %dx%d ordinal %s group (%d, %d, %d)%s seed %d" % (N, Cn, c.Ks[0], c.Ks[1], c.ordinal, c.Mg, c.m0, c.M, " greedy" if c.greedy else "", c.seed)
        if c.kind == "rows":
            out = _sample(hip, c, "cadre_sample_rows")
            worst = max(worst, _check_group(c, out, "cadre_sample_rows " + tag))
            marked = _sample(hip, c, "cadre_sample_rows_ord", np.full((2, 64), -1, np.int32))
            for g, m, name in zip(out, marked, ("action", "logp", "value")):
                assert np.array_equal(g.view(np.uint8), m.view(np.uint8)), "cadre_sample_rows_ord under the -1 marker: %s differs from the plain entry point (%s)" % (name, tag)
        elif c.kind == "ord":
            worst = max(worst, _check_group(c, _sample(hip, c, "cadre_sample_rows_ord", c.tables), "cadre_sample_rows_ord " + tag))
        else:
            table = c.tables if any(c.ordinal) else None
            worst = max(worst, _check_group(c, _sample(hip, c, "cadre_sample_rows_ens", table), "cadre_sample_rows_ens " + tag))
            if N >= 5:                                             # out-of-range cmd / pos: the header promises a skip (for _ens only)
                bad = [(1, "cmd", Cn), (3, "pos", N), (4, "cmd", -1)]
                keep = np.ones(N, bool)
                keep[[1, 3, 4]] = False
                _check_group(c, _sample(hip, c, "cadre_sample_rows_ens", table, bad), "cadre_sample_rows_ens (3 environments out of range) " + tag, keep)
    print("step-parity B2 N %d C %d: worst err / bound = %.3f" % (N, Cn, worst))
