"""GPU: the six fused kernels of the PPO minibatch update (cadre_amd/csrc/ppo_update.hip) through the C ABI against float64 on the operands as
stored, EVERY element of every net's run, at the bound of tests/update_parity.py: stage-wise |got - y64| <= c_bar 2^-24 mag with c_bar from the
CPU (the sequential fp32 chain of the case's own products, doubled, under K + 5), the gates inside the enclosure of their pre-activation's
slack widened by T_ACT / T_TANH ulps, h_t bit-identical to the product of its stored factors, outputs without magnitude exact zeros.
Shapes: the smallest that reach every path (one / two live tiles of the last chunk, one-row tails, empty runs, unsorted rows, D = 37,
k-step counts of the weight-gradient pipeline that are no multiple of its depth, partial column groups).  Two heads of two command nets
(Z = 4, C = 2) whose runs differ, unless a case is cut to one head to keep its CPU chain short.  Every case prints one line per output
kind: excess (units) <= c_bar <= cap, or the ulps outside the enclosure next to the worst OBSERVED ulp distance where the argument is known
exactly.  What tests/test_kernels_gpu.py asserts on the same kernels (untouched rows, foreign rows, repeatability) is not repeated."""
import ctypes

import numpy as np
import pytest
import torch

from tests import update_parity as up

pytestmark = pytest.mark.gpu

DP = 544                                                   # ldh: the hidden width 530 zero padded, built into the kernels
NB = 34                                                    # k-blocks of 16 in DP


def dev(x):
    return torch.as_tensor(x).cuda()


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def pad(t, w, fill=0.0):
    out = torch.full(tuple(t.shape[:-1]) + (w,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def pack(hip, W, D):
    """W [Z][4D][D] -> the two fragment-order copies of cadre_pack_lstm_weights, [2][Z][NP]."""
    Z = W.shape[0]
    NP = (D + 15) // 16 * 4 * NB * 256
    Wd = dev(pad(W, DP))
    packed = torch.zeros(2, Z, NP, device="cuda")
    hip.check(hip.lib().cadre_pack_lstm_weights(Wd.data_ptr(), 4 * D * DP, DP, D, Z, packed[0].data_ptr(), packed[1].data_ptr(), NP, hip.stream()),
              "cadre_pack_lstm_weights")
    return packed, NP


def spans(runs, B, Z):
    """[(first, count)] per net or None -> [(lo, hi)] per net."""
    return [(0, B)] * Z if runs is None else [(lo, min(B, lo + n)) for lo, n in runs]


# (name, Z, B, D, runs per net (None: unsorted), saturate, rev)
STEP_CASES = [
    ("B64 runs 17+47 | 16+48", 4, 64, 530, [(0, 17), (17, 47), (0, 16), (16, 48)], False, 0),
    ("B80 runs 33+47", 2, 80, 530, [(0, 33), (33, 47)], True, 1),
    ("B80 runs 49+31", 2, 80, 530, [(0, 49), (49, 31)], False, 0),
    ("B20 empty run", 4, 20, 530, [(0, 0), (0, 20), (0, 0), (0, 20)], False, 0),
    ("B1 unsorted", 4, 1, 530, None, False, 1),
    ("B24 unsorted", 2, 24, 530, None, False, 0),
    ("D37 B24 runs 7+17 | 24+0", 4, 24, 37, [(0, 7), (7, 17), (0, 24), (24, 0)], True, 1),
]


@pytest.mark.parametrize("name,Z,B,D,runs,saturate,rev", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_lstm_step_fwd(hip, name, Z, B, D, runs, saturate, rev):
    """cadre_lstm_step_fwd: gates in the enclosure of Gx + h W^T + b, c_t within 3 units of its stored factors, tanh(c_t) within T_TANH ulps,
    h_t bit-identical."""
    r = np.random.RandomState(1000 + B + D)
    W, b, Gx, hp, cp = up.lstm_fwd_operands(r, Z, B, D, saturate)
    H4 = 4 * D
    ldg = (H4 + 63) // 64 * 64
    packed, NP = pack(hip, W, D)
    bd = dev(b)
    Gd = dev(pad(Gx, ldg, 7.0))
    hpd, cpd = dev(pad(hp, DP)), dev(pad(cp, DP))
    ho = torch.full((Z, B, DP), 7.0, device="cuda")
    co, tco = torch.full_like(ho, 7.0), torch.full_like(ho, 7.0)
    segd = None if runs is None else dev(torch.tensor(runs, dtype=torch.int32))
    hip.check(hip.lib().cadre_lstm_step_fwd(packed[0].data_ptr(), NP, bd.data_ptr(), H4, Gd.data_ptr(), ldg, B * ldg, hpd.data_ptr(), cpd.data_ptr(),
                                            ho.data_ptr(), co.data_ptr(), tco.data_ptr(), DP, B * DP, B, D, Z,
                                            None if segd is None else segd.data_ptr(), rev, hip.stream()), "cadre_lstm_step_fwd")
    torch.cuda.synchronize()
    G, h, c, tc = Gd.cpu(), ho.cpu(), co.cpu(), tco.cpu()
    case = up.Case("lstm_step_fwd %s" % name)
    for z, (lo, hi) in enumerate(spans(runs, B, Z)):
        if hi > lo:
            got = dict(act=G[z, lo:hi, :H4].contiguous(), c=c[z, lo:hi, :D], tc=tc[z, lo:hi, :D], h=h[z, lo:hi, :D])
            up.lstm_fwd_check(case, W[z], b[z], Gx[z, lo:hi], hp[z, lo:hi], cp[z, lo:hi], got)
    case.finish()
    print("lstm_step_fwd %s: c_bar of the pre-activation %.3f <= cap %d" % (name, case.pre_cb, up.DIRECT_CAP(D + 2)))


def frag(t, runs, B, H4):
    """[Z][B][H4] -> the fragment order of the backward's A operand, [Z][tile][k-block][q][r16][i]: 16-row tiles counted from the first row of
    the net's run (NaN where no row lives), the gate axis zero padded to 2176."""
    Z = t.shape[0]
    Bp = (B + 15) // 16 * 16
    full = torch.full((Z, Bp, 4 * DP), float("nan"))
    full[:, :, H4:] = 0
    for z, (lo, hi) in enumerate(spans(runs, B, Z)):
        full[z, :hi - lo, :H4] = t[z, lo:hi]
    return full.view(Z, Bp // 16, 16, 4 * NB, 4, 4).permute(0, 1, 3, 4, 2, 5).contiguous()


@pytest.mark.parametrize("name,Z,B,D,runs,saturate,rev", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_lstm_step_bwd(hip, name, Z, B, D, runs, saturate, rev):
    """cadre_lstm_step_bwd with and without the product: dG_{t-1} and dc within (c_bar_dh + c_poly) units of the float64 polynomial on
    (value, magnitude) pairs, on the rows a net owns (sorted: its run; unsorted: the rows of its command)."""
    C = 2
    r = np.random.RandomState(2000 + B + D)
    W = torch.from_numpy(r.standard_normal((Z, 4 * D, D)).astype(np.float32) * np.float32(0.04 if D > 100 else 0.15))
    dG_t, dh_in, dc, cp, tc, act = up.lstm_bwd_operands(r, Z, B, D, saturate)
    H4 = 4 * D
    ldg = (H4 + 63) // 64 * 64
    cmds = torch.from_numpy(r.randint(0, C, (Z // C, B)).astype(np.int32))
    if runs is not None:                                   # rows sorted by command: consistent with the runs
        for z, (lo, hi) in enumerate(spans(runs, B, Z)):
            cmds[z // C, lo:hi] = z % C
    own = torch.stack([cmds[z // C] == z % C for z in range(Z)])
    packed, NP = pack(hip, W, D)
    dGt_d = dev(frag(dG_t, runs, B, H4))
    gps = dGt_d[0].numel()
    act_d, tcd, cpd, dhd, cm = dev(pad(act, ldg)), dev(pad(tc, DP)), dev(pad(cp, DP)), dev(pad(dh_in, DP)), dev(cmds)
    segd = None if runs is None else dev(torch.tensor(runs, dtype=torch.int32))
    for with_product in (1, 0):
        dGo = torch.full((Z, B, ldg), 7.0, device="cuda")
        dGpo = torch.full_like(dGt_d, 7.0)
        dCd = dev(pad(dc, DP))
        hip.check(hip.lib().cadre_lstm_step_bwd(packed[1].data_ptr(), NP, dGt_d.data_ptr() if with_product else None, dGpo.data_ptr(), gps,
                                                dGo.data_ptr(), act_d.data_ptr(), ldg, B * ldg, dhd.data_ptr(), dCd.data_ptr(), B * DP,
                                                tcd.data_ptr(), cpd.data_ptr(), DP, B * DP, B, D, Z, cm.data_ptr(), C,
                                                None if segd is None else segd.data_ptr(), rev, hip.stream()), "cadre_lstm_step_bwd")
        torch.cuda.synchronize()
        dG, dCo = dGo.cpu(), dCd.cpu()
        case = up.Case("lstm_step_bwd %s product %d" % (name, with_product))
        for z, (lo, hi) in enumerate(spans(runs, B, Z)):
            rows = torch.arange(lo, hi)[own[z, lo:hi]]
            if len(rows):
                up.lstm_bwd_check(case, W[z], dG_t[z, rows], dh_in[z, rows], act[z, rows], tc[z, rows], cp[z, rows], dc[z, rows],
                                  dG[z, rows, :H4], dCo[z, rows, :D], with_product)
        case.finish()
        print("lstm_step_bwd %s product %d: c_bar_dh %.3f <= cap %d, c_poly %.3f <= N_POLY %d"
              % (name, with_product, case.cb_dh, up.DIRECT_CAP(H4) if with_product else 0, case.c_poly, up.N_POLY))


# (name, Z, B, S, H4, N, ldg, ldh, ldw, runs per net)
DW_SMALL = [("B7 runs 1+6 | 7+0", 7, [(0, 1), (1, 6), (0, 7), (7, 0)]), ("B19 runs 5+14 | 14+5", 19, [(0, 5), (5, 14), (0, 14), (14, 5)])]
DW_CASES = [("%s S%d" % (n, S), 4, B, S, 130, 76, 192, 80, 76, runs) for n, B, runs in DW_SMALL for S in (1, 3, 5)] + \
           [("B19 runs 5+14 S3 full width", 2, 19, 3, 2120, 544, 2176, 544, 544, [(0, 5), (5, 14)])]


@pytest.mark.parametrize("name,Z,B,S,H4,N,ldg,ldh,ldw,runs", DW_CASES, ids=[c[0] for c in DW_CASES])
def test_lstm_dw(hip, name, Z, B, S, H4, N, ldg, ldh, ldw, runs):
    """cadre_lstm_dw: dW_hh, dW_ih and db of every net, every element, k-step counts nb * S that are no multiple of the pipeline depth 4
    (run lengths 1, 5, 6, 7, 14 and 0; S = 1, 3, 5), H4 = 130 (a last m-group with two live rows), N = 76 (a partial second n-group).
    Rows of other nets and stale rows hold NaN."""
    C = 2
    r = np.random.RandomState(3000 + B + S + H4)
    rn = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    own = up.runs_own(runs, B)
    Nd = min(N, 530)                                        # columns past the hidden width are zero padding
    dG = pad(rn(Z, S, B, H4), ldg)
    Hs, X = pad(pad(rn(Z, S + 1, B, Nd), N), ldh), pad(pad(rn(Z // C, S, B, Nd), N), ldh)
    sL = 2 * H4 * ldw + 2 * H4
    assert sL % 4 == 0 and (H4 * ldw) % 4 == 0
    grads = torch.full((Z * sL,), 7.0, device="cuda")
    dGd, Hsd, Xd = dev(dG), dev(Hs), dev(X)
    foreign = (~own).cuda()[:, None].expand(Z, S, B)
    dGd[foreign] = float("nan")
    Hsd[:, :S][foreign] = float("nan")
    segd = dev(torch.tensor(runs, dtype=torch.int32))
    hip.check(hip.lib().cadre_lstm_dw(dGd.data_ptr(), ldg, S * B * ldg, Hsd.data_ptr(), Xd.data_ptr(), ldh, (S + 1) * B * ldh, S * B * ldh, C,
                                      grads.data_ptr() + 4 * H4 * ldw, grads.data_ptr(), grads.data_ptr() + 4 * 2 * H4 * ldw,
                                      grads.data_ptr() + 4 * (2 * H4 * ldw + H4), ldw, sL, B, S, H4, N, Z, segd.data_ptr(), hip.stream()), "cadre_lstm_dw")
    torch.cuda.synchronize()
    out = grads.cpu().view(Z, sL)
    ih, hh = out[:, :H4 * ldw].view(Z, H4, ldw), out[:, H4 * ldw:2 * H4 * ldw].view(Z, H4, ldw)
    b_ih, b_hh = out[:, 2 * H4 * ldw:2 * H4 * ldw + H4], out[:, 2 * H4 * ldw + H4:]
    case = up.Case("lstm_dw %s" % name)
    for z, (lo, hi) in enumerate(spans(runs, B, Z)):
        dY = dG[z, :, lo:hi, :H4].reshape(-1, H4)
        Ys = [Hs[z, :S, lo:hi, :N].reshape(-1, N), X[z // C, :, lo:hi, :N].reshape(-1, N)]
        up.dw_check(case, "dW_hh, dW_ih, db", dY, Ys, [hh[z, :, :N], ih[z, :, :N]], b_ih[z])
    case.add_bits("db_hh == db_ih", b_hh, b_ih)
    case.finish()


# (name, B, runs per net (None: unsorted, Z = 4 nets))
MLP_CASES = [("B49 runs 1+15+16+17+0", 49, [(0, 1), (1, 15), (16, 16), (32, 17), (49, 0)]), ("B5 unsorted", 5, None)]


@pytest.mark.parametrize("name,B,runs", MLP_CASES, ids=[c[0] for c in MLP_CASES])
def test_mlp_towers(hip, name, B, runs):
    """cadre_mlp_fwd / cadre_mlp_bwd / cadre_mlp_dw, each stage against float64 of the STORED results of the stage before: A1, A2, O3; dA2, dA1
    (exact zeros under the ReLU masks), dH over both towers of a net (exact zeros in the padding columns); the six gradients per tower (exact
    zeros for a net without rows and in W1's padding columns).  Rows outside a run hold NaN."""
    Z = 4 if runs is None else len(runs)
    Z2, D, hid, NP = 2 * Z, 530, 128, 64
    r = np.random.RandomState(4000 + B)
    rn = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    n_out = ([33, 1] * 2 + [3, 1] * 3)[:Z2]
    t_w1, t_b1 = 0, hid * DP
    t_w2, t_b2 = t_b1 + hid, t_b1 + hid + hid * hid
    t_w3, t_b3 = t_b2 + hid, t_b2 + hid + NP * hid
    sT = t_b3 + NP
    offs = (ctypes.c_int32 * 6)(t_w1, t_b1, t_w2, t_b2, t_w3, t_b3)
    W1, b1 = pad(rn(Z2, hid, D) * 0.05, DP), rn(Z2, hid) * 0.1
    W2, b2 = rn(Z2, hid, hid) * 0.1, rn(Z2, hid) * 0.1
    W3, b3, dO3 = torch.zeros(Z2, NP, hid), torch.zeros(Z2, NP), torch.zeros(Z2, B, NP)
    for z2 in range(Z2):
        W3[z2, :n_out[z2]], b3[z2, :n_out[z2]] = rn(n_out[z2], hid) * 0.1, rn(n_out[z2]) * 0.1
        dO3[z2, :, :n_out[z2]] = rn(B, n_out[z2]) * 0.3
    P = torch.cat([torch.cat([W1[z].reshape(-1), b1[z], W2[z].reshape(-1), b2[z], W3[z].reshape(-1), b3[z]]) for z in range(Z2)])
    assert P.numel() == Z2 * sT and sT % 4 == 0
    H = pad(rn(Z, B, D), DP)
    own = torch.ones(Z, B, dtype=torch.bool) if runs is None else up.runs_own(runs, B)
    own2 = own.repeat_interleave(2, 0)
    nan_rows = lambda t, o: torch.where(o[..., None].expand_as(t), t, torch.full_like(t, float("nan")))
    Pd, Hd, dO3d = dev(P), dev(nan_rows(H, own)), dev(nan_rows(dO3, own2))
    A1 = torch.full((Z2, B, hid), 7.0, device="cuda")
    A2, O3 = torch.full_like(A1, 7.0), torch.full((Z2, B, NP), 7.0, device="cuda")
    dA1, dA2, dH = torch.full_like(A1, 7.0), torch.full_like(A1, 7.0), torch.full((Z, B, DP), 7.0, device="cuda")
    G = torch.full((Z2 * sT,), 7.0, device="cuda")
    L = hip.lib()
    sp = None if runs is None else dev(torch.tensor(runs, dtype=torch.int32))
    spp = None if sp is None else sp.data_ptr()
    hip.check(L.cadre_mlp_fwd(Pd.data_ptr(), sT, offs, Hd.data_ptr(), DP, B * DP, A1.data_ptr(), A2.data_ptr(), O3.data_ptr(), B, Z2, spp, hip.stream()),
              "cadre_mlp_fwd")
    hip.check(L.cadre_mlp_bwd(Pd.data_ptr(), sT, offs, dO3d.data_ptr(), A1.data_ptr(), A2.data_ptr(), dA1.data_ptr(), dA2.data_ptr(), dH.data_ptr(),
                              DP, B * DP, B, Z2, spp, hip.stream()), "cadre_mlp_bwd")
    hip.check(L.cadre_mlp_dw(dO3d.data_ptr(), dA2.data_ptr(), dA1.data_ptr(), A2.data_ptr(), A1.data_ptr(), Hd.data_ptr(), DP, B * DP, G.data_ptr(), sT,
                             offs, B, Z2, spp, hip.stream()), "cadre_mlp_dw")
    torch.cuda.synchronize()
    A1, A2, O3, dA1, dA2, dH = (t.cpu() for t in (A1, A2, O3, dA1, dA2, dH))
    Gv = G.cpu().view(Z2, sT)
    case = up.Case("mlp towers %s" % name)
    par = lambda z2, w1: (w1, b1[z2], W2[z2], b2[z2], W3[z2], b3[z2])
    for z, (lo, hi) in enumerate(spans(runs, B, Z)):
        rows = slice(lo, hi)
        for z2 in (2 * z, 2 * z + 1):
            if hi > lo:
                up.mlp_fwd_check(case, H[z, rows, :D], par(z2, W1[z2, :, :D]), dict(A1=A1[z2, rows], A2=A2[z2, rows], O3=O3[z2, rows]))
            g = Gv[z2]
            got = (g[t_w1:t_b1].view(hid, DP), g[t_b1:t_w2], g[t_w2:t_b2].view(hid, hid), g[t_b2:t_w3], g[t_w3:t_b3].view(NP, hid), g[t_b3:])
            up.mlp_dw_check(case, dO3[z2, rows], dA2[z2, rows], dA1[z2, rows], A2[z2, rows], A1[z2, rows], H[z, rows], got)
        if hi > lo:
            tw = slice(2 * z, 2 * z + 2)
            up.mlp_bwd_check(case, dO3[tw, rows], A1[tw, rows], A2[tw, rows], par(2 * z, W1[2 * z]), par(2 * z + 1, W1[2 * z + 1]),
                             dict(dA2=dA2[tw, rows], dA1=dA1[tw, rows], dH=dH[z, rows]))
    case.finish()
