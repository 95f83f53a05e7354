"""Element-wise float64 parity for the two pieces of the step path the earlier parity modules left out — the bound, stated once
("fp32 parity": the row-segment descriptors; "loss / head / optimiser parity": the act chain).  No bar is new: the products
answer to tests/f32_parity.py (|got - y64| <= c_bar 2^-24 mag, c_bar from f32_parity.c_bar_direct — the sequential fp32 chain of the
case's own products over EVERY output whose magnitude is not zero, doubled, asserted under DIRECT_CAP(K) = K + 5), the sampling launches to
the running first-order bound of tests/loss_parity.py (front_reference, candidates, Report).  Nothing is taken from a kernel's output.

A. Row-segment descriptors of cadre_gemm_f32 (seg_mode 1, 2, 3 of cadre_amd/csrc/gemm_f32.hip), built as cadre_amd/learner.py builds them:

    A1  learner.py:944-947   the LSTM input projection of the update: NT product, a_z = (x_div, 0, S*B*DP), per-net weights and bias,
                             seg = (3, seg, B, 1) — compact rows, period B
    A2  cadre_amd/ppo_agent/agent.py:400-423   the same launch from act_batch: period N = the number of environments (any value from 1),
                             x_div = 2C (every net reads head block 0), the table from ppo_agent.agent.command_rows
    A3  learner.py:1191-1198 layer_bwd: dW = dY^T X (a_mode = b_mode = 1, seg = (2, seg, B, 2): k-tiles), dX = dY W (b_mode 1,
                             seg = (1, seg, B, 2): M tiles);  learner.py:1214-1217: the two towers into dH (seg = (1, seg, B, 1), the
                             second launch accumulates in place: resid is C)

A descriptor is a SegDesc in SLOT form: every operand is a tensor [slots][rows][ld], the batch triple (div, mod, stride) of cadre_gemm_t
keeps its (div, mod) and the stride is the tensor's.  For one descriptor this module gives the five things a test needs:

    own_rows(d, z)      the rows batch entry z owns — of C in modes 1 and 3, of the K axis in mode 2.  Mode 3: the run of every period
                        (compact row mc = (mc / cnt) period + beg + mc % cnt: ascending).  Mode 1: every row of every M tile that meets
                        the run in its period; the unit is the M tile the kernel used (tile_rows: cadre_gemm_pick_tile and the fallback
                        at gemm_f32.hip:704), and every row of an owned tile is a full product
    entry(d, z, ops)    the float64 value y, the magnitude mag (|A||B| + |bias| + |resid|), the product groups for fp.c_bar_direct
    c_bar(d, e)         fp.c_bar_direct over the outputs with mag > 0 (idx=, as tests/update_parity.py), the case inside DIRECT_BUDGET
    untouched(d, ...)   the mask of the elements of the C buffer the launch must leave as they are: foreign rows, ldc padding columns,
                        the tiles of empty runs (a margin behind the buffer is the caller's: MARGIN floats)
    check_case(...)     all of it for every batch entry, through update_parity.Case: one printed `excess <= c_bar <= cap` line

Mode 2 multiplies only the k-tiles of the run; the callers keep the foreign rows of dY exact zeros, so the reference is the product over ALL
K = S * period rows (a zero product adds no error in either arithmetic) and the cap DIRECT_CAP(S * period).  An empty net: exact zeros.

emulate3 is the mode-3 launch in fp32 numpy (strictly sequential, or in 32-term chunks) with its mutants, for tests/test_step_parity_cpu.py.

B. The act chain.  RingModel is cadre_act_windows (cadre_amd/csrc/act_batch.hip) in numpy, exact: the ring shifted or refilled, the rows
latent | np.float32(measurements) x 6 | +0 written to X[s][pos[e]] and feat[e][s].  SampleCase holds one launch of cadre_sample_rows / _ord /
_ens: the tower buffer O3 with finite junk in its padding, q, and per head the pairs (lg, score) of loss_parity.front_reference on exactly
the rows the kernel must read; check_sample asserts the action inside loss_parity.candidates, logp inside the bound, the value's bits.

Plain helper module (no GPU, no fixtures)."""
import numpy as np
import torch

from tests import f32_parity as fp
from tests import loss_parity as lp
from tests import update_parity as up

F4, F8 = np.float32, np.float64
FILL = 7.0                 # what the C buffers are filled with before a launch
MARGIN = 4096              # floats behind every buffer that must keep the fill
# rows of the M tile per tile id (include/cadre_hip.h, cadre_gemm_t.tile)
TILE_BM = {1: 128, 2: 128, 3: 64, 4: 256, 5: 128, 6: 256, 8: 128, 9: 32, 10: 128}


def slot(z, zt):
    """operand slot of batch entry z under the triple (div, mod, ..): (z / div) % mod, mod 0 = not reached."""
    q = z // max(1, zt[0])
    return q % zt[1] if zt[1] > 0 else q


def tile_rows(picked, mode, period):
    """M-tile rows of the launch: `picked` = cadre_gemm_pick_tile's answer, then the fallback of gemm_f32.hip:704 (seg_mode 1: the M tile
    must divide the period, else 64 rows where 64 divides it, else 32)."""
    bm = TILE_BM[picked]
    if mode == 1 and period % bm != 0:
        bm = 64 if period % 64 == 0 else 32
    return bm


class SegDesc:
    """One row-segment descriptor in slot form.  M, N, K as cadre_gemm_t has them; S periods of `period` rows on the segmented axis (M in
    modes 1 and 3, K in mode 2); seg int [n][2] = (first row, count); bm: rows of the M tile (mode 1)."""

    def __init__(self, mode, seg, period, seg_div, S, Z, N, K=None, M=None, ldc=None, a_mode=0, b_mode=0, a_z=(1, 0), b_z=(1, 0), c_z=(1, 0),
                 s_z=(1, 0), r_z=(1, 0), act=0, bm=None, what=""):
        self.mode, self.seg, self.period, self.seg_div, self.S, self.Z = mode, np.asarray(seg, np.int64).reshape(-1, 2), period, seg_div, S, Z
        self.M = S * period if mode != 2 else M
        self.K = S * period if mode == 2 else K
        self.N, self.ldc = N, N if ldc is None else ldc
        self.a_mode, self.b_mode, self.a_z, self.b_z, self.c_z, self.s_z, self.r_z = a_mode, b_mode, a_z, b_z, c_z, s_z, r_z
        self.act, self.bm, self.what = act, bm, what
        assert mode in (1, 2, 3) and (mode != 1 or (bm and period % bm == 0)) and self.seg.shape[0] * seg_div >= Z

    def run(self, z):
        beg, cnt = self.seg[z // self.seg_div]
        return int(beg), int(cnt)


def own_rows(d, z):
    """Ascending int64 rows of the segmented axis that batch entry z owns (module docstring)."""
    beg, cnt = d.run(z)
    if cnt <= 0:
        return np.zeros(0, np.int64)
    if d.mode == 1:
        t0 = np.arange(0, d.period, d.bm)
        live = t0[(t0 + d.bm > beg) & (t0 < beg + cnt)]
        r = (live[:, None] + np.arange(d.bm)[None, :]).reshape(-1)
    else:
        r = np.arange(beg, beg + cnt)
    return (np.arange(d.S)[:, None] * d.period + r[None, :]).reshape(-1).astype(np.int64)


def _operands(d, z, ops, rows):
    """-> (Az [m][K], Bm [N][K], shift [N] or None, resid [m][N] or None) of batch entry z as the float64 reference takes them."""
    A, B = ops["A"][slot(z, d.a_z)], ops["B"][slot(z, d.b_z)]
    Az = A[:, :d.K] if d.a_mode == 0 else A[:d.K, :d.M].t()
    Bm = B[:d.N, :d.K] if d.b_mode == 0 else B[:d.K, :d.N].t()
    shift = None if ops.get("bias") is None else ops["bias"][slot(z, d.s_z)][:d.N]
    res = None if ops.get("resid") is None else ops["resid"][slot(z, d.r_z)][:, :d.N]
    if d.mode != 2:
        r = torch.from_numpy(rows)
        Az, res = Az[r], None if res is None else res[r]
    return Az.contiguous(), Bm.contiguous(), shift, None if res is None else res.contiguous()


def entry(d, z, ops):
    """One batch entry -> dict(rows = the C rows it writes, y, mag [rows][N] float64, groups, shift, resid, K), or None where it writes
    nothing (an empty run in modes 1 and 3)."""
    rows = own_rows(d, z)
    if d.mode == 2:
        rows = np.arange(d.M, dtype=np.int64)                    # every row of dW is written; an empty net gives zeros
    if rows.size == 0:
        return None
    Az, Bm, shift, res = _operands(d, z, ops, rows)
    acc, mac = fp.dense_acc(Az, Bm)
    y, mag = fp.epilogue32(acc, mac, None, shift, res, d.act)
    return dict(rows=rows, y=y, mag=mag, groups=[fp.dense_products(Az, Bm)], shift=shift, resid=res, K=Az.shape[1])


def c_bar(d, e, what=""):
    """-> (c_bar or None where no output has a magnitude, cap): fp.c_bar_direct over every output with mag > 0."""
    K = e["K"]
    assert e["y"].numel() * K <= fp.DIRECT_BUDGET, "%s: choose a shape whose every chain can be summed" % what
    live = np.flatnonzero(e["mag"].reshape(-1).numpy() > 0).astype(np.int64)
    if live.size == 0:
        return None, fp.DIRECT_CAP(K)
    return fp.c_bar_direct(e["groups"], e["y"], e["mag"], None, e["shift"], e["resid"], d.act, what=what, idx=live)


def untouched(d, c_slots, c_rows):
    """bool [c_slots][c_rows][ldc]: the elements of the C buffer no batch entry may write."""
    m = np.ones((c_slots, c_rows, d.ldc), bool)
    for z in range(d.Z):
        rows = np.arange(d.M) if d.mode == 2 else own_rows(d, z)
        m[slot(z, d.c_z), rows, :d.N] = False
    return m


def reference(d, ops):
    """Every batch entry's entry() with its c_bar: [(z, e or None, cb, cap)] — computed once per case, shared by the tiles."""
    out = []
    for z in range(d.Z):
        e = entry(d, z, ops)
        cb, cap = (None, fp.DIRECT_CAP(d.K)) if e is None else c_bar(d, e, "%s z=%d" % (d.what, z))
        out.append((z, e, cb, cap))
    return out


def check_case(d, ref, got, fill, what):
    """got: the whole C buffer after the launch, fp32 tensor [c_slots][c_rows][ldc] (+ nothing else); fill: the same buffer as it was
    before.  Every owned element under the bound (one c_bar per case: the largest over the entries), every other element bit for bit as
    filled.  -> (excess, c_bar, cap)."""
    g, f = got.numpy(), fill.numpy()
    keep = untouched(d, g.shape[0], g.shape[1])
    bad = keep & (g.view(np.uint32) != f.view(np.uint32))
    assert not bad.any(), "%s: %d elements outside the rows the entries own were written (first at %s)" % (
        what, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))
    case = up.Case(what)
    for z, e, cb, cap in ref:
        if e is None:
            continue
        rows = torch.from_numpy(e["rows"])
        case.add_units("C", got[slot(z, d.c_z)][rows][:, :d.N], e["y"], e["mag"], cb, cap)
    st = case.finish()
    return st.get("C")


# ----------------------------------------------------------------------------- mode 3 in fp32 numpy (CPU teeth)
def emulate3(d, ops, order="seq", mut=None):
    """The seg_mode 3 launch on the CPU: C [Z][M][ldc] fp32 (FILL where nothing is written); products rounded to fp32, summed strictly
    sequentially ("seq") or in 32-term chunks ("chunk": one k-tile each, added to the running sum), + bias.  Mutants: "trunc16" / "trunc19"
    (both operands cut to that many mantissa bits), "bias_next" (the bias of net z + 1), "no_period" (the compact-row map without its
    t * period term), "tail_row" (the last row of entry 0's run in the last period reads its last four k from the next row of A),
    "drop" (row 0 of every entry loses its last product)."""
    assert d.mode == 3 and d.a_mode == 0 and d.b_mode == 0
    C = np.full((d.Z, d.M, d.ldc), FILL, F4)
    q = (lambda t: fp.trunc_mantissa(t, int(mut[5:]))) if mut in ("trunc16", "trunc19") else (lambda t: t)
    hit = False
    for z in range(d.Z):
        rows = own_rows(d, z)
        if rows.size == 0:
            continue
        src = rows % d.period + (0 if mut == "no_period" else rows // d.period * d.period)
        A = ops["A"][slot(z, d.a_z)]
        Az = q(A[torch.from_numpy(src), :d.K]).numpy().copy()
        if mut == "tail_row" and not hit and src[-1] + 1 < A.shape[0]:
            Az[-1, -4:] = A[int(src[-1]) + 1, d.K - 4:d.K].numpy()
            hit = True
        Bm = q(ops["B"][slot(z, d.b_z)][:d.N, :d.K]).numpy()
        P = Az[:, None, :] * Bm[None, :, :]
        if mut == "drop":
            P[0, :, -1] = 0
        acc = fp._chain(P, 32 if order == "chunk" else 1)
        bz = z + 1 if mut == "bias_next" else z
        v = acc + ops["bias"][slot(bz % d.Z, d.s_z)][:d.N].numpy()[None, :]
        assert v.dtype == F4
        C[slot(z, d.c_z), src if mut == "no_period" else rows, :d.N] = v
    assert mut != "tail_row" or hit
    return torch.from_numpy(C)


def measure_case(d, ref, got):
    """The bound's statistics of a whole C buffer against `ref` without asserting (for mutants): -> (failures list, old metric)."""
    gs, ys, ms, cbs, cap = [], [], [], [], 0
    for z, e, cb, cp in ref:
        if e is None:
            continue
        gs.append(got[slot(z, d.c_z)][torch.from_numpy(e["rows"])][:, :d.N].reshape(-1))
        ys.append(e["y"].reshape(-1))
        ms.append(e["mag"].reshape(-1))
        cbs.append(cb or 0.0)
        cap = max(cap, cp)
    g, y, m = torch.cat(gs), torch.cat(ys), torch.cat(ms)
    st = fp.measure(g, y, m, max(cbs), None, out_f32=True)
    return fp.failures(st, out_f32=True), fp.old_metric(g, y), st


def seg_operands(r, d, a_slots, a_rows, lda, b_slots, bias=True, w_scale=0.05):
    """Random operands of an NT descriptor (modes 1 / 3 with a_mode = b_mode = 0): A ~ N(0, 1) [a_slots][a_rows][lda], W ~ w_scale N(0, 1)
    [b_slots][N][K], bias ~ N(0, 1) [b_slots][N]."""
    rn = lambda shape, s=1.0: torch.from_numpy((r.standard_normal(shape) * s).astype(F4))
    return dict(A=rn((a_slots, a_rows, lda)), B=rn((b_slots, d.N, d.K), w_scale), bias=rn((b_slots, d.N)) if bias else None)


# ----------------------------------------------------------------------------- the cases (shared by the CPU and the GPU tests)
Z_NETS, C_CMDS, DP = 8, 4, 544             # 2 heads x 4 command nets; the LSTM input width 530 padded to 544 = K
T100 = ([[3, 1], [4, 37], [41, 59], [100, 0]], [[0, 33], [33, 30], [63, 0], [63, 37]])
# (N, ldc, S, B, head 0's runs, head 1's runs).  Across the list: empty runs, one-row runs ([3, 1], [63, 1], [40, 1]), a run that is the whole
# period ([0, 96]), runs that start and end off every multiple of 32 ([4, 37], [33, 14], [41, 55]), the two heads' tables different, runs that
# leave rows of the period to nobody (case 1: rows 26 .. 32 and 47 .. 63 of head 0), B = 100 no multiple of 32
A1_CASES = [(2120, 2176, 1, 100) + T100,
            (2120, 2176, 3, 64, [[5, 1], [6, 20], [26, 0], [33, 14]], [[0, 13], [13, 0], [13, 22], [40, 9]]),
            (96, 96, 3, 96, [[0, 0], [0, 96], [96, 0], [96, 0]], [[0, 10], [10, 30], [40, 1], [41, 55]]),
            (96, 96, 1, 64, [[0, 16], [16, 16], [32, 31], [63, 1]], [[7, 50], [57, 0], [57, 3], [60, 4]]),
            (96, 96, 3, 100) + T100]
A1_TILES = (0, 3, 8, 9)


def a1_case(i):
    """Case i of A1_CASES -> (SegDesc, operands): learner.py:944-947 with x_div = C — X [2 heads][S * B][DP], W [8][N][DP], bias [8][N]."""
    N, ldc, S, B, t0, t1 = A1_CASES[i]
    d = SegDesc(3, t0 + t1, B, 1, S, Z_NETS, N, K=DP, ldc=ldc, a_z=(C_CMDS, 0), what="mode 3 update form N %d ldc %d S %d B %d" % (N, ldc, S, B))
    return d, seg_operands(np.random.RandomState(300 + i), d, 2, S * B, DP, Z_NETS)


# (period N, S, commands): all environments on one command; commands without an environment; orders whose pos is not the identity
A2_CMDS = {1: [2], 5: [2, 0, 2, 1, 0], 17: [3, 1, 0, 3, 3, 1, 0, 0, 3, 1, 3, 0, 1, 1, 3, 0, 3], 32: [1] * 32,
           "5one": [3] * 5, "32mix": [(7 * i * i + 3 * i) % 5 % 4 if i % 6 else 3 for i in range(32)]}
A2_CASES = [(1, 1, 1, 2120, 2176), (1, 2, 1, 2120, 2176), (5, 1, 5, 2120, 2176), (5, 2, "5one", 2120, 2176), (17, 1, 17, 2120, 2176),
            (17, 2, 17, 2120, 2176), (32, 1, 32, 2120, 2176), (32, 2, "32mix", 2120, 2176), (5, 2, 5, 96, 96), (17, 2, 17, 96, 96)]
A2_TILES = (0, 3, 9)


def a2_case(i, draw=0):
    """Case i of A2_CASES -> (SegDesc, operands, pos): agent.py:400-423 — the table from command_rows, period = the number of environments,
    x_div = 2C: every net reads block 0 of X [2][S * N][DP]; block 1 is NaN (a net that read it would show).  draw: another draw of the
    operands for the same descriptor (tests/test_step_parity_cpu.py)."""
    from ppo_agent.agent import command_rows
    n, S, key, N, ldc = A2_CASES[i]
    cmds = A2_CMDS[key]
    assert len(cmds) == n
    pos, seg = command_rows(cmds, C_CMDS)
    d = SegDesc(3, seg, n, 1, S, Z_NETS, N, K=DP, ldc=ldc, a_z=(2 * C_CMDS, 0), what="mode 3 act form N %d ldc %d S %d envs %d (%s)" % (N, ldc, S, n, key))
    ops = seg_operands(np.random.RandomState(400 + i + 100 * draw), d, 2, S * n, DP, Z_NETS)
    ops["A"][1] = float("nan")
    return d, ops, pos


# the shapes of test_gemm_row_segments (tests/test_kernels_gpu.py): Z = 4 nets, S = 2, 96 x 64, the period's table
A3_CASES = [(128, [[0, 40], [40, 0], [40, 70], [110, 18]]), (96, [[0, 10], [10, 30], [40, 0], [40, 56]]), (64, [[0, 16], [16, 16], [32, 31], [63, 1]])]
A3_TILES = (0, 3, 9)
A3_Z, A3_S, A3_NY, A3_NX = 4, 2, 96, 64


def _rn(r, shape, s=1.0):
    return torch.from_numpy((r.standard_normal(shape) * s).astype(F4))


def a3_dw(i):
    """learner.py:1193-1194: dW[z] = dY[z]^T X[z / 2] over the S * P rows, z = 2 net + tower; the rows of dY outside the net's run are
    exact zeros, as cadre_relu_bwd leaves them.  -> (SegDesc, operands: A = dY [8][S P][96], B = X [4][S P][64])."""
    P, seg = A3_CASES[i]
    d = SegDesc(2, seg, P, 2, A3_S, 2 * A3_Z, A3_NX, M=A3_NY, a_mode=1, b_mode=1, b_z=(2, 0), what="mode 2 dW = dY^T X P %d" % P)
    r = np.random.RandomState(500 + i)
    dY, X = _rn(r, (2 * A3_Z, A3_S * P, A3_NY)), _rn(r, (A3_Z, A3_S * P, A3_NX))
    for z in range(2 * A3_Z):
        keep = torch.zeros(A3_S * P, dtype=torch.bool)
        keep[torch.from_numpy(own_rows(d, z))] = True
        dY[z][~keep] = 0.0
    return d, dict(A=dY, B=X)


def a3_dx(i, bm):
    """learner.py:1197-1198: dX[z] = dY[z] W[z] (W k-major [96][64]), seg = (1, seg, P, 2).  dY is dense here: every row of an owned
    tile is a full product and is checked as one."""
    P, seg = A3_CASES[i]
    d = SegDesc(1, seg, P, 2, A3_S, 2 * A3_Z, A3_NX, K=A3_NY, b_mode=1, bm=bm, what="mode 1 dX = dY W P %d BM %d" % (P, bm))
    r = np.random.RandomState(600 + i)
    return d, dict(A=_rn(r, (2 * A3_Z, A3_S * P, A3_NY)), B=_rn(r, (2 * A3_Z, A3_NY, A3_NX), 0.1))


def a3_dh(i, bm):
    """learner.py:1214-1217: dH[z] = dA1[2 z] W1[2 z] + dA1[2 z + 1] W1[2 z + 1] in two launches, seg = (1, seg, P, 1), the second with
    resid = C.  -> (SegDesc, full operands A [4][2][S P][64], B [4][2][64][96]); tower t's launch takes A[:, t], B[:, t]."""
    P, seg = A3_CASES[i]
    d = SegDesc(1, seg, P, 1, A3_S, A3_Z, A3_NY, K=A3_NX, b_mode=1, bm=bm, what="mode 1 two towers into dH P %d BM %d" % (P, bm))
    r = np.random.RandomState(700 + i)
    return d, dict(A=_rn(r, (A3_Z, 2, A3_S * P, A3_NX)), B=_rn(r, (A3_Z, 2, A3_NX, A3_NY), 0.1))


# ----------------------------------------------------------------------------- A4: the glue launches
def colsum_reference(X, prev, accumulate, what=""):
    """cadre_colsum of a whole launch: X [batch][M][N], prev [batch][N] -> (y [1][batch * N], mag, c_bar, cap): the product of a row of
    ones with every column (one c_bar over all batch entries: a single entry of three columns can be exact throughout), the previous
    content as the residual when accumulating."""
    batch, M, N = X.shape
    res = prev.reshape(1, batch * N).contiguous() if accumulate else None
    return up.direct(torch.ones(1, M), X.permute(0, 2, 1).reshape(batch * N, M).contiguous(), resid=res, what=what)


def relu_bwd_reference(act, dy, commands=None, B=0, hid=0, C=0):
    """cadre_relu_bwd on flat fp32 arrays: the kept elements keep their bits, the others are +0."""
    keep = act > 0
    if commands is not None:
        row = np.arange(act.size) // hid
        b, net = row % B, (row // B) >> 1
        keep = keep & (np.asarray(commands).reshape(-1)[(net // C) * B + b] == net % C)
    return np.where(keep, dy, F4(0.0)).astype(F4)


# ----------------------------------------------------------------------------- B1: cadre_act_windows
LAT, NMEAS = 512, 18


def window_firsts(modes, S):
    """first[] as act_batch lays it out: the fresh frames of all environments in one array, one frame of a shifted window, S of a reset one.
    -> (first int32 [N], number of fresh frames)."""
    first, nf = [], 0
    for m in modes:
        first.append(nf)
        nf += 1 if m else S
    return np.asarray(first, np.int32), nf


class RingModel:
    """cadre_act_windows on numpy arrays, exact.  ring [n_ring][ring_env_str] fp32, slot e = environment e's window [S][512]."""

    def __init__(self, n_ring, S, ring_env_str, fill):
        assert ring_env_str >= S * LAT
        self.S, self.ring = S, np.full((n_ring, ring_env_str), fill, F4)

    def step(self, fresh, mode, first, meas, pos, DP, X, feat=None):
        """fresh [F][ld_fresh] fp32; mode, first, pos int [N]; meas float64 [N][S][3]; X [S][N][ldx] and feat [N][S][ldf] (or None) are
        written in place on their first DP columns."""
        S, N = self.S, len(mode)
        for e in range(N):
            win = self.ring[e, :S * LAT].reshape(S, LAT)
            if mode[e]:
                win[:-1] = win[1:].copy()
                win[-1] = fresh[first[e], :LAT]
            else:
                win[:] = fresh[first[e]:first[e] + S, :LAT]
            row = np.zeros((S, DP), F4)
            row[:, :LAT] = win
            row[:, LAT:LAT + NMEAS] = np.tile(np.asarray(meas[e], F8).astype(F4), (1, NMEAS // 3))
            X[:, pos[e], :DP] = row
            if feat is not None:
                feat[e, :, :DP] = row
        return X, feat


def awkward_measurements(r, N, S):
    """float64 [N][S][3] that are no fp32 numbers: random values, and per environment one just above a rounding tie (1 + 2^-24 + 2^-40
    times a power of two: rounds up to nearest, down under truncation), one just below (rounds down, up under round-away), one negative."""
    m = r.standard_normal((N, S, 3)) * 10.0 ** r.uniform(-3, 3, (N, S, 3))
    tie = 1.0 + 2.0 ** -24
    for e in range(N):
        m[e, 0, 0] = (tie + 2.0 ** -40) * 2.0 ** (e % 7)
        m[e, S - 1, 1] = (tie - 2.0 ** -40) * 2.0 ** -(e % 5)
        m[e, S // 2, 2] = -(tie + 2.0 ** -40) * 3.0
    assert (m.astype(F4).astype(F8) != m).all()
    return m


# ----------------------------------------------------------------------------- B2: cadre_sample_rows / _ord / _ens
class SampleCase:
    """One sampling launch.  N environments with commands `cmds` (pos from command_rows), C commands, Mg group agents m0 .. m0 + Mg - 1 of M,
    Ks = (K_steer, K_throttle), ordinal = per head.  O3 [4 Mg C][z_str] fp32: actor tower z = 2 (h Mg C + j C + c), row p at p * ldo, K logits
    from loss_parity.raw_rows (every net its own draw), junk behind them and in the gap behind the N rows; the critic tower z + 1 holds a
    value in column 0.  q [N][M][2][64] fp32 = exponential + 1e-3, 1.0 in the lanes >= K; greedy: q is not passed (the reference divides by 1).
    bad: environments whose cmd / pos the caller puts out of range before the launch (they must keep the fill): left out of the reference."""

    def __init__(self, seed, cmds, C, Ks, ordinal=(False, False), Mg=1, m0=0, M=1, ldo=72, gap=40, greedy=False, kind="rows"):
        from ppo_agent.agent import command_rows
        r = np.random.RandomState(seed)
        self.kind, self.seed = kind, seed
        self.cmds = np.asarray(cmds, np.int32)
        self.N, self.C, self.Ks, self.ordinal, self.Mg, self.m0, self.M = len(cmds), C, Ks, ordinal, Mg, m0, M
        self.ldo, self.greedy = ldo, greedy
        N = self.N
        self.pos, self.seg = command_rows(list(cmds), C)
        self.z_str = N * ldo + gap
        nz = 4 * Mg * C
        O3 = (r.standard_normal((nz, self.z_str)) * 3.0 + 11.0).astype(F4)            # finite junk everywhere first
        self.tables = np.stack([lp.rank_table(Ks[h], ordinal[h]) for h in range(2)])
        for h in range(2):
            for n in range(Mg * C):
                z = 2 * (h * Mg * C + n)
                rows = lp.raw_rows(r, N, Ks[h], 4.0, ordinal[h])
                O3[z, :N * ldo].reshape(N, ldo)[:, :Ks[h]] = rows
                O3[z + 1, :N * ldo].reshape(N, ldo)[:, 0] = r.standard_normal(N).astype(F4)
        self.O3 = O3
        q = np.ones((N, M, 2, 64), F4)
        for h in range(2):
            q[:, :, h, :Ks[h]] = r.exponential(1.0, (N, M, Ks[h])).astype(F4) + F4(1e-3)
        self.q = q

    def tower(self, h, j, e):
        return 2 * (h * self.Mg * self.C + j * self.C + int(self.cmds[e]))

    def rows(self, h, row_of=None, tower_of=None):
        """raw fp32 [N * Mg][K_h] in (e, j) order: what the pair (e, j, h) reads.  row_of / tower_of: mutants."""
        K, out = self.Ks[h], []
        for e in range(self.N):
            for j in range(self.Mg):
                z = self.tower(h, j, e) if tower_of is None else tower_of(h, j, e)
                p = int(self.pos[e]) if row_of is None else row_of(e)
                out.append(self.O3[z, p * self.ldo:p * self.ldo + K])
        return np.stack(out)

    def q_rows(self, h):
        K = self.Ks[h]
        if self.greedy:
            return np.ones((self.N * self.Mg, K), F4)
        return self.q[:, self.m0:self.m0 + self.Mg, h, :K].reshape(self.N * self.Mg, K)

    def values(self, h):
        return np.array([self.O3[self.tower(h, j, e) + 1, int(self.pos[e]) * self.ldo] for e in range(self.N) for j in range(self.Mg)], F4)

    def reference(self, h):
        """-> (x, lg pairs [N Mg][K], score pairs, candidates, equal = the rows of all-equal categorical logits) of head h."""
        x = self.rows(h)
        rk = self.tables[h][:self.Ks[h]].astype(np.int64) if self.ordinal[h] else None
        X, lg, pk, _H = lp.front_reference(x, rk)
        score = (pk / X.sum(pk)[..., None]) / lp.VE(self.q_rows(h))
        equal = (x == x[:, :1]).all(-1) & (not self.ordinal[h])
        return x, lg, score, lp.candidates(score), equal

    def ambiguous(self):
        """Pairs with more than one candidate, the all-equal categorical rows of a greedy launch left aside (planted ties: index 0 wins)."""
        n = 0
        for h in range(2):
            _x, _lg, _sc, cand, equal = self.reference(h)
            n += int(((cand.sum(-1) > 1) & ~(equal & self.greedy)).sum())
        return n

    def emulate(self, order="tree", mut=(), row_of=None, tower_of=None):
        """The kernel's statements in fp32 numpy (loss_parity.X32) -> action int64, logp fp32, value fp32, each [N][Mg][2]."""
        act, logp, val = (np.zeros((self.N, self.Mg, 2), t) for t in (np.int64, F4, F4))
        X = lp.X32(order)
        for h in range(2):
            x = self.rows(h, row_of, tower_of)
            rk = self.tables[h][:self.Ks[h]].astype(np.int64) if self.ordinal[h] else None
            lg, pk, _H, _s, _t = lp.front(X, x, rk, mut)
            sc = (pk / X.sum(pk)[..., None]) / self.q_rows(h)
            a = np.argmax(sc, -1)                                  # (the first of equal maxima: the lowest index)
            act[:, :, h] = a.reshape(self.N, self.Mg)
            logp[:, :, h] = lg[np.arange(len(a)), a].reshape(self.N, self.Mg)
            val[:, :, h] = self.values(h).reshape(self.N, self.Mg)
        return act, logp, val


SAMPLE_N, SAMPLE_C, SAMPLE_KS = (1, 5, 17, 32), (1, 4), ((33, 3), (64, 1), (1, 64))
SAMPLE_GROUPS = ((1, 0, 1), (2, 1, 4), (4, 0, 4))                   # (Mg, m0, M), Mg * C <= 16


def sample_cases(N=None, C=None):
    """The launches of B2 as SampleCase keyword sets: kind "rows" (cadre_sample_rows, and cadre_sample_rows_ord under the -1 marker on both
    heads: the same bits), "ord" (both heads ordinal; steer only), "ens" (the three groups, q given and greedy, plain and steer-ordinal
    alternating).  The seeds are fixed here; tests/test_step_parity_cpu.py asserts the ambiguity cap for every one of them."""
    out = []
    for n in SAMPLE_N if N is None else (N,):
        for c in SAMPLE_C if C is None else (C,):
            key = {1: 1, 5: 5, 17: 17, 32: "32mix"}[n]
            cmds = [0] * n if c == 1 else A2_CMDS[key]
            for k, Ks in enumerate(SAMPLE_KS):
                base = dict(cmds=cmds, C=c, Ks=Ks)
                seed = 1000 * n + 100 * c + 10 * k
                out.append(dict(base, seed=seed, kind="rows"))
                out.append(dict(base, seed=seed + 1, kind="ord", ordinal=(True, True)))
                out.append(dict(base, seed=seed + 2, kind="ord", ordinal=(True, False)))
                for g, (Mg, m0, M) in enumerate(SAMPLE_GROUPS):
                    for greedy in (False, True):
                        out.append(dict(base, seed=seed + 3 + 2 * g + greedy, kind="ens", Mg=Mg, m0=m0, M=M, greedy=greedy,
                                        ordinal=((k + g) % 2 == 1, False)))
    return out


def check_sample(case, act, logp, val, what, keep_env=None, quiet=False):
    """act int64, logp, val fp32 [N][Mg][2] of the group's agents, in environment order.  keep_env: bool [N], the environments that must
    have been written (default all).  -> (worst err / bound, ambiguous pairs); raises on any violation."""
    N, Mg = case.N, case.Mg
    env = np.ones(N, bool) if keep_env is None else np.asarray(keep_env)
    live = np.repeat(env, Mg)
    rep = lp.Report(what)
    n_amb = 0
    for h in range(2):
        K = case.Ks[h]
        _x, lg, score, cand, equal = case.reference(h)
        a = np.asarray(act)[:, :, h].reshape(-1)
        n = np.arange(N * Mg)
        assert ((a[live] >= 0) & (a[live] < K)).all(), "%s head %d: an action outside 0 .. %d" % (what, h, K - 1)
        ac = np.where(live, a, 0)
        assert cand[n, ac][live].all(), "%s head %d: a sampled index outside the candidates" % (what, h)
        sure = cand.sum(-1) == 1
        assert (ac[sure & live] == np.argmax(score.v, -1)[sure & live]).all(), "%s head %d: not the float64 argmax on an unambiguous row" % (what, h)
        if case.greedy:
            assert (ac[equal & live] == 0).all(), "%s head %d: a row of equal logits did not pick index 0" % (what, h)
        n_amb += int(((~sure) & live & ~(equal & case.greedy)).sum())
        rep.check("logp head %d" % h, np.asarray(logp)[:, :, h].reshape(-1), lg[n, ac], live)
        want = case.values(h)
        got = np.ascontiguousarray(np.asarray(val, F4)[:, :, h].reshape(-1))
        bad = (got.view(np.uint32) != want.view(np.uint32)) & live
        assert not bad.any(), "%s head %d: %d values are not the bits of the critic tower (first at pair %d)" % (what, h, int(bad.sum()), int(np.argmax(bad)))
    rep.finish(n_amb, quiet)
    return rep.worst, n_amb
