"""GPU: self-imitation learning (csrc/selfimit.hip, cadre_amd/selfimit.py).

  1  all rows kind 0: cadre_ppo_sil_loss is cadre_ppo_loss_ord bit for bit (losses, gradients, the stats row, the gate flag, the block)
  2  a mixed minibatch: the PPO rows' gradients are the PPO kernel's, the SIL rows' those of an all-SIL launch, bit for bit
  3  every stored element against float64 at the running bound of tests/loss_parity.py (tests/selfimit_parity.py), the four variants
  4  the KL gate and the PPO diagnostics see the PPO rows only
  5  cadre_sil_prepare against cadre_gae_multi (tau = 1, V = 0) and the numpy statements, both tail settings
  6  cadre_sil_draw against the numpy draw, exactly
  7  cadre_sil_scatter against the numpy statement
  8  end to end through learner_section_multi and train_vec"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import demo_mix_ref
from tests import selfimit_parity as sp
from tests import selfimit_ref as ref
from tests.loss_parity import F4, SENT, XVE
from tests.test_demo_mix_gpu import CC, CLIP, EC, FP, NS, NT, VC, dev_inputs, head_args, head_rows, hp_block, mix_case, run_ppo, table_of
from tests.test_loss_parity_gpu import DECOY, F_PPO, Launch, dev, host

pytestmark = pytest.mark.gpu
SC, SVC = 0.7, 0.3
FS = 6
ALPHA, EPS = 0.6, 1e-3
# (B, B_ppo, C): B 24 with 12 / 0 / 24 SIL rows, B 300 with 77
CASES = [(24, 12, 4), (24, 24, 1), (24, 0, 4), (300, 223, 4)]


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def sil_block(**over):
    from cadre_amd import hip as h
    hp = hp_block(**over)
    hp[h.HP_SIL_COEFF], hp[h.HP_SIL_VALUE_COEFF] = SC, SVC
    return hp


def new_outputs(B, C):
    nblk = (B + 15) // 16
    f = lambda shape, v: torch.full(shape, v, device="cuda")
    out = dict(losses=f((3,), 7.0), sil_losses=f((2,), 7.0), sil_w=f((2, B), 7.0), dl=f((2 * C, B, 64), 9.0), dv=f((2 * C, B), 9.0),
               scratch=f((4 + 6 * nblk,), 3.0), sil_scratch=f((2 * nblk * (2 + FS),), 3.0), stats=f((2, FP), 5.0),
               sscr=f((12 * nblk,), 3.0), sil_stats=f((2, FS), 5.0), stop=torch.zeros(1, dtype=torch.int32, device="cuda"))
    out["scratch"][0] = 0.0                                # the arrival counter: zero on first use, reset by every launch
    return out


def run_sil(d, o, B, C, table, inv_b, inv_bs, hp=None, stats=False, sstats=True, target_kl=0.0, coeffs=(SC, SVC)):
    from cadre_amd import hip as h
    h.check(h.lib().cadre_ppo_sil_loss(
        *head_args(d, B, C), d["old_v"].data_ptr(), d["rets"].data_ptr(), d["old_lp"].data_ptr(), d["adv"].data_ptr(),
        d["kind"].data_ptr(), B, C, NS, NT, None if hp is None else hp.data_ptr(), CLIP, VC, CC, EC, inv_b, coeffs[0], coeffs[1],
        inv_bs, o["losses"].data_ptr(), o["sil_losses"].data_ptr(), o["sil_w"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(),
        o["scratch"].data_ptr(), o["sil_scratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None, FP,
        o["sscr"].data_ptr() if stats else None, target_kl, o["stop"].data_ptr() if stats else None,
        o["sil_stats"].data_ptr() if sstats else None, FS, None if table is None else table.data_ptr(), h.stream()),
        "cadre_ppo_sil_loss")
    assert float(o["scratch"][0]) == 0.0                   # the counter is left zero
    return o


def scales(B, B_ppo):
    return 1.0 / max(B_ppo, 1), 1.0 / max(B - B_ppo, 1)


# ----------------------------------------------------------------------------- 1. all rows kind 0
@pytest.mark.parametrize("ordinal", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_all_ppo_rows_is_the_ppo_kernel(case, ordinal):
    """Every output equals cadre_ppo_loss_ord's on the same inputs, in the four variants (stats x hp): losses, gradients, the stats row,
    the stop flag and the block's lr after the KL-adaptive rule (a gate that fires and one that does not); the SIL outputs are zeros."""
    from cadre_amd import hip as h
    B, _bp, C = case
    inp, ranks = mix_case(B, _bp, C)
    d = dev_inputs(inp, kind=torch.zeros(2, B, dtype=torch.int32), actions=inp["actions"].clamp(min=0))
    table = table_of(ranks, ordinal)
    for tkl in (1e-6, 1e3):
        hp_m, hp_p = (sil_block(desired_kl=1e-5, lr_min=1e-5, lr_max=1e-2, lr_factor=1.5) for _ in range(2))
        mix = run_sil(d, new_outputs(B, C), B, C, table, 1.0 / B, 1.0, hp=hp_m, stats=True, target_kl=tkl, coeffs=(DECOY, DECOY))
        ppo = run_ppo(d, new_outputs(B, C), B, C, table, 1.0 / B, hp=hp_p, stats=True, target_kl=tkl)
        assert all(torch.equal(mix[k], ppo[k]) for k in ("losses", "dl", "dv", "stop")) and torch.equal(hp_m, hp_p)
        assert torch.equal(mix["stats"][:, :7], ppo["stats"][:, :7])            # (field 7 belongs to cadre_grad_norms_hp)
        assert int(mix["stop"]) == (1 if tkl < 1 else 0) and float(mix["stats"][0, 6]) == (0.0 if tkl < 1 else 1.0)
        assert (float(hp_m[h.HP["lr"]]) == 3e-4) == (tkl < 1)
        assert float(mix["sil_losses"].abs().max()) == 0.0 and float(mix["sil_stats"].abs().max()) == 0.0
        assert float(mix["sil_w"].abs().max()) == 0.0
        by_val = run_sil(d, new_outputs(B, C), B, C, table, 1.0 / B, 1.0, stats=True, target_kl=tkl)
        want = run_ppo(d, new_outputs(B, C), B, C, table, 1.0 / B, stats=True, target_kl=tkl)
        assert all(torch.equal(by_val[k], want[k]) for k in ("losses", "dl", "dv", "stop"))
        assert torch.equal(by_val["stats"][:, :7], want["stats"][:, :7])
    for hp in (None, sil_block()):
        plain = run_sil(d, new_outputs(B, C), B, C, table, 1.0 / B, 1.0, hp=hp)
        want = run_ppo(d, new_outputs(B, C), B, C, table, 1.0 / B, hp=None if hp is None else sil_block())
        assert all(torch.equal(plain[k], want[k]) for k in ("losses", "dl", "dv")) and float((plain["stats"] - 5.0).abs().max()) == 0.0


# ----------------------------------------------------------------------------- 2. a mixed minibatch
@pytest.mark.parametrize("layout", ["prefix", "random"])
@pytest.mark.parametrize("ordinal", [False, True])
@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
def test_rows_are_the_ppo_kernel_and_the_all_sil_launch_bit_for_bit(case, ordinal, layout):
    B, B_ppo, C = case
    inp, ranks = mix_case(B, B_ppo, C, layout)
    inv_b, inv_bs = scales(B, B_ppo)
    d, table = dev_inputs(inp), table_of(ranks, ordinal)
    mix = run_sil(d, new_outputs(B, C), B, C, table, inv_b, inv_bs)
    mix_hp = run_sil(d, new_outputs(B, C), B, C, table, inv_b, inv_bs, hp=sil_block(), coeffs=(DECOY, DECOY))
    mix_st = run_sil(d, new_outputs(B, C), B, C, table, inv_b, inv_bs, hp=sil_block(), stats=True, coeffs=(DECOY, DECOY))
    mix_sv = run_sil(d, new_outputs(B, C), B, C, table, inv_b, inv_bs, stats=True)
    ppo = run_ppo(d, new_outputs(B, C), B, C, table, inv_b)
    all_sil = run_sil(dev_inputs(inp, kind=torch.ones(2, B, dtype=torch.int32)), new_outputs(B, C), B, C, table, 1.0, inv_bs)
    assert bool(torch.isfinite(mix["dl"]).all()) and bool(torch.isfinite(mix["dv"]).all())
    for other in (mix_hp, mix_st, mix_sv):
        assert all(torch.equal(other[k], mix[k]) for k in ("losses", "sil_losses", "sil_w", "dl", "dv", "sil_stats"))
    assert torch.equal(mix_st["stats"], mix_sv["stats"])
    for hd in range(2):
        p = torch.nonzero(d["kind"][hd] == 0).view(-1)
        q = torch.nonzero(d["kind"][hd] != 0).view(-1)
        assert torch.equal(head_rows(mix["dl"], hd, C, p), head_rows(ppo["dl"], hd, C, p))
        assert torch.equal(head_rows(mix["dv"], hd, C, p), head_rows(ppo["dv"], hd, C, p))
        assert torch.equal(head_rows(mix["dl"], hd, C, q), head_rows(all_sil["dl"], hd, C, q))
        assert torch.equal(head_rows(mix["dv"], hd, C, q), head_rows(all_sil["dv"], hd, C, q))
        assert torch.equal(mix["sil_w"][hd, q], all_sil["sil_w"][hd, q]) and float(mix["sil_w"][hd, p].abs().max()) == 0.0
        assert float(head_rows(mix["dl"], hd, C, p).abs().max()) > 0 and float(head_rows(mix["dl"], hd, C, q).abs().max()) > 0
        # a SIL row with a bad command or no action gets exact zeros in all C nets
        cq, aq = d["cmds"][hd][q], d["actions"][hd][q]
        out = q[(cq < 0) | (cq >= C) | (aq < 0)]
        assert out.numel() == 3 and float(head_rows(mix["dl"], hd, C, out).abs().max()) == 0.0
        assert float(head_rows(mix["dv"], hd, C, out).abs().max()) == 0.0 and float(mix["sil_w"][hd, out].abs().max()) == 0.0
    first = {k: mix[k].clone() for k in ("losses", "sil_losses", "sil_w", "dl", "dv", "sil_stats")}
    for _ in range(3):                                     # partials combine in workgroup order: equal inputs give equal bits
        run_sil(d, mix, B, C, table, inv_b, inv_bs)
        assert all(torch.equal(mix[k], first[k]) for k in first)


# ----------------------------------------------------------------------------- 3. every stored element against float64
class SilLaunch(Launch):
    def outputs(self):
        o = Launch.outputs(self)
        c = self.c
        o.update(sil_losses=torch.full((8,), float(SENT), device="cuda"), sil_w=torch.full((2, c.B), float(SENT), device="cuda"),
                 sil_stats=torch.zeros(2, FS, device="cuda"), sil_scratch=torch.full((2 * self.nblk * (2 + FS),), 3.0, device="cuda"))
        return o

    def sil(self, o, use_hp, stats, kinds):
        c, L, hp = self.c, self.hip.lib(), self.c.hp
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        coeffs = [float(hp["sil_coeff"]), float(hp["sil_value_coeff"])]
        block = self.block().clone()
        block[self.hip.HP_SIL_COEFF], block[self.hip.HP_SIL_VALUE_COEFF] = coeffs
        head = self.head() + [kinds.data_ptr(), c.B, c.C, c.Ks[0], c.Ks[1]]
        rc = L.cadre_ppo_sil_loss(*head, block.data_ptr() if use_hp else None, *([DECOY] * 4 if use_hp else byval), float(hp["inv_b"]),
                                  *([DECOY] * 2 if use_hp else coeffs), float(hp["inv_bs"]), o["losses"].data_ptr(),
                                  o["sil_losses"].data_ptr(), o["sil_w"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(),
                                  o["scratch"].data_ptr(), o["sil_scratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None,
                                  F_PPO, o["sscratch"].data_ptr() if stats else None, 0.0, None,
                                  o["sil_stats"].data_ptr() if stats else None, FS, self.ord.data_ptr() if any(c.ordinal) else None,
                                  self.hip.stream())
        self.hip.check(rc, "cadre_ppo_sil_loss")
        got = self.collect(o, stats)
        assert bool((o["sil_losses"][2:] == float(SENT)).all()), "a SIL loss beyond its slot was written"
        got.update(sil_losses=host(o["sil_losses"])[:2], sil_w=host(o["sil_w"]))
        if stats:
            got["sil_stats"] = host(o["sil_stats"])
        return got


@pytest.mark.parametrize("i", range(len(sp.SIL_CASES)), ids=lambda i: "B%d-sil%d-C%d" % (
    sp.SIL_CASES[i]["B"], sp.SIL_ROWS[sp.SIL_CASES[i]["B"]][sp.SIL_CASES[i]["demo_share"]], sp.SIL_CASES[i]["C"]))
def test_every_stored_element_against_float64(hip, i):
    """dlogits, dvalues, sil_w, the PPO and SIL losses and both statistics rows within the running first-order bound (T_EXP, T_LOG of
    tests/loss_parity.py; no other tolerance), rows with R <= v exact zeros, untouched sentinels still sentinels — by value and with the
    block, with and without statistics.  The kinds come from cadre_mix_row_kinds on the case's sorted layout."""
    c = sp.sil_case(sp.SIL_CASES[i])
    run = SilLaunch(hip, c)
    kinds = torch.full((2, c.B), 9, dtype=torch.int32, device="cuda")
    pos = dev(c.pos)
    hip.check(hip.lib().cadre_mix_row_kinds(pos.data_ptr(), c.B, c.B_ppo, kinds.data_ptr(), hip.stream()), "cadre_mix_row_kinds")
    assert np.array_equal(host(kinds), c.kindrow)
    want = sp.run_sil(c, XVE)
    for use_hp, stats in ((False, False), (False, True), (True, False), (True, True)):
        got = run.sil(run.outputs(), use_hp, stats, kinds)
        _w, n_amb = sp.check_sil(c, got, want, "cadre_ppo_sil_loss hp %s stats %d %s" % ("block" if use_hp else "NULL", stats, c.tag()),
                                 stats=stats)
        assert n_amb <= 1
        if stats and c.B_ppo < c.B:
            n_rows = [c.rows(h, True).size for h in range(2)]
            assert got["sil_stats"][:, 5].tolist() == [float(n) for n in n_rows]


# ----------------------------------------------------------------------------- 4. the gate sees the PPO rows only
def test_kl_gate_and_diagnostics_see_the_ppo_rows_only():
    """SIL rows whose old_logp / old_values / adv slots would wreck the KL if read: every output is bit for bit that of a launch with
    harmless values there; the PPO statistics are those of the PPO rows alone in float64; target_kl just above / below their KL flips
    `applied` and the stop flag."""
    B, B_ppo, C = 24, 12, 4
    inp, ranks = mix_case(B, B_ppo, C, "random")
    inv_b, inv_bs = scales(B, B_ppo)
    t = lambda a: a.clone()
    out = demo_mix_ref.ppo_rows_loss(inp["logits"].double(), inp["values"].double(), inp["actions"], inp["cmds"], inp["old_v"].double(),
                                     inp["rets"].double(), inp["old_lp"].double(), inp["adv"].double(), inp["kind"], (NS, NT), (None, None),
                                     C, CLIP, VC, CC, EC, inv_b)
    want_st = out[4]
    sil = inp["kind"] != 0
    bad = dict(old_lp=torch.where(sil, torch.full_like(inp["old_lp"], -1000.0), inp["old_lp"]),
               old_v=torch.where(sil, torch.full_like(inp["old_v"], 1e30), inp["old_v"]),
               adv=torch.where(sil, torch.full_like(inp["adv"], float("nan")), inp["adv"]))
    table = table_of(ranks, False)
    good = run_sil(dev_inputs(inp), new_outputs(B, C), B, C, table, inv_b, inv_bs, stats=True, target_kl=1e3)
    poisoned = run_sil(dev_inputs(inp, **bad), new_outputs(B, C), B, C, table, inv_b, inv_bs, stats=True, target_kl=1e3)
    assert all(torch.equal(poisoned[k], good[k]) for k in ("losses", "sil_losses", "sil_w", "dl", "dv", "stats", "sil_stats", "stop"))
    assert float((poisoned["stats"][:, :6].double().cpu() - want_st).abs().max()) < 1e-5 and int(poisoned["stop"]) == 0
    assert float(poisoned["stats"][0, 6]) == 1.0
    kl = float(want_st[:, 0].max())
    assert kl > 1e-3
    for factor, applied in ((0.99, 0.0), (1.01, 1.0)):     # the gate: max KL > 1.5 target_kl
        o = run_sil(dev_inputs(inp, **bad), new_outputs(B, C), B, C, table, inv_b, inv_bs, stats=True, target_kl=factor * kl / 1.5)
        assert float(o["stats"][0, 6]) == applied and float(o["stats"][1, 6]) == applied and int(o["stop"]) == 1 - int(applied)


# ----------------------------------------------------------------------------- 5. cadre_sil_prepare
T_P, G32 = 16, float(np.float32(0.99))


def prep_storages(seed, tl_null):
    """8 storages (4 mask patterns x 2 heads): no end; an end at the last row; two ends; an end with the time-limit flag (and a true end
    before it).  Returns flat host arrays [8][T + 1]."""
    r = np.random.RandomState(seed)
    n, P = 8, T_P + 1
    rew = r.standard_normal((n, P)).astype(F4)
    val = (0.5 * r.standard_normal((n, P))).astype(F4)
    masks, tl = np.ones((n, P), F4), np.zeros((n, P), F4)
    for h in range(2):
        masks[2 + h, T_P - 1] = 0
        masks[4 + h, 4 + h] = masks[4 + h, 11] = 0
        masks[6 + h, 3] = 0
        masks[6 + h, 9 + h] = 0
        tl[6 + h, 9 + h] = 1
    if tl_null:
        tl[:] = 0
    return rew, masks, tl, val


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("tail", ["drop", "bootstrap"])
def test_prepare_against_the_scan_and_the_numpy_statements(hip, tail, scaled):
    L, n, P, T = hip.lib(), 8, T_P + 1, T_P
    rew, masks, tl, val = prep_storages(5 + scaled, tl_null=False)
    d = {k: dev(v.copy()) for k, v in dict(rew=rew, masks=masks, tl=tl, val=val).items()}
    R = torch.full((n, P), 7.0, device="cuda")
    flags = torch.full((n, P), 9, dtype=torch.int32, device="cuda")
    q = torch.full((n, P), 9, dtype=torch.int32, device="cuda")
    state, clip_r = None, 0.0
    if scaled:
        st = np.zeros(8 + 2 * n)
        st[hip.RS_SCALE], st[hip.RS_SCALE + 1] = float(F4(0.37)), float(F4(1.9))
        state, clip_r = dev(st), 1.25
    row = lambda t, k: t.data_ptr() + 4 * P * k
    table = dev(np.array([[row(d["rew"], k), row(d["masks"], k), row(d["tl"], k), row(d["val"], k), row(R, k), row(flags, k), row(q, k)]
                          for k in range(n)], np.int64))
    hip.check(L.cadre_sil_prepare(table.data_ptr(), n, T, G32, None if state is None else state.data_ptr(), clip_r,
                                  ["drop", "bootstrap"].index(tail), ALPHA, EPS, hip.stream()), "cadre_sil_prepare")
    # the yardstick: cadre_gae_multi with tau = 1 (gamma_tau = gamma), V = 0, next_value = 0
    zeros, nv = torch.zeros(n, P, device="cuda"), torch.zeros(n, device="cuda")
    ret, adv = torch.zeros(n, P, device="cuda"), torch.zeros(n, T, device="cuda")
    gtab = dev(np.array([[row(d["rew"], k), row(zeros, k), row(d["masks"], k), nv.data_ptr() + 4 * k, row(ret, k), adv.data_ptr() + 4 * T * k,
                          row(d["tl"], k)] for k in range(n)], np.int64))
    hip.check(L.cadre_gae_multi(gtab.data_ptr(), n, T, G32, G32, 0, None if state is None else state.data_ptr(), clip_r, hip.stream()),
              "cadre_gae_multi")
    Rg, fl, qg, scan = host(R), host(flags), host(q), host(ret)
    assert np.array_equal(host(d["val"]), val) and np.array_equal(host(d["rew"]), rew)      # inputs untouched
    assert np.all(Rg[:, T] == 7.0)                                                          # returns[T] is not written
    n_closed = 0
    for k in range(n):
        sc = None if not scaled else (0.37 if k % 2 == 0 else 1.9)
        Rn, fn = ref.closed_scan(rew[k], masks[k], tl[k], val[k], G32, tail, scale=sc, clip_r=clip_r if scaled else None)
        assert np.array_equal(fl[k], fn), (k, fl[k], fn)
        closed = (fn[:T] & 1) != 0
        n_closed += int(closed.sum())
        assert np.array_equal(Rg[k, :T][closed].view(np.uint32), scan[k, :T][closed].view(np.uint32)), k       # bit-equal to the scan
        assert np.array_equal(Rg[k, :T].view(np.uint32), Rn.view(np.uint32)), k                                 # and to the numpy statement
        want_q = ref.initial_priorities(Rn, fn, val[k], ALPHA, EPS)
        elig = (fn & 2) != 0
        assert np.all(qg[k][~elig] == 0) and qg[k][T] == 0 and np.all(qg[k][elig] >= 1)
        assert np.abs(qg[k].astype(np.int64) - want_q).max() <= 1, k
        if tail == "drop":
            assert np.array_equal(elig[:T], closed)
        else:
            assert elig[:T].all()
    # the patterns: nothing closed, everything closed, rows 0 .. 11 closed, rows 0 .. 3 closed (the flagged end closes nothing)
    want_closed = [0, 0, T, T, 12, 12, 4, 4]
    assert [int(((fl[k, :T] & 1) != 0).sum()) for k in range(n)] == want_closed and n_closed == sum(want_closed)


def test_prepare_without_time_limits_pointer(hip):
    """time_limits 0 in the record: the scan without flags (keep = 1), equal to a launch with an all-zero flag array."""
    L, n, P, T = hip.lib(), 8, T_P + 1, T_P
    rew, masks, tl, val = prep_storages(9, tl_null=True)
    d = {k: dev(v.copy()) for k, v in dict(rew=rew, masks=masks, tl=tl, val=val).items()}
    outs = []
    for with_ptr in (True, False):
        R, flags, q = torch.zeros(n, P, device="cuda"), torch.zeros(n, P, dtype=torch.int32, device="cuda"), torch.zeros(n, P, dtype=torch.int32, device="cuda")
        row = lambda t, k: t.data_ptr() + 4 * P * k
        table = dev(np.array([[row(d["rew"], k), row(d["masks"], k), row(d["tl"], k) if with_ptr else 0, row(d["val"], k), row(R, k),
                               row(flags, k), row(q, k)] for k in range(n)], np.int64))
        hip.check(L.cadre_sil_prepare(table.data_ptr(), n, T, G32, None, 0.0, 1, ALPHA, EPS, hip.stream()), "cadre_sil_prepare")
        outs.append((host(R), host(flags), host(q)))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


# ----------------------------------------------------------------------------- 6. cadre_sil_draw
@functools.lru_cache(maxsize=None)
def draw_table(Rcap):
    """Priorities [2][Rcap] with runs of zeros, one row at the cap and small values; a filled count below Rcap (Rcap > 1)."""
    r = np.random.RandomState(Rcap)
    q = r.randint(1, 1 << 20, (2, Rcap)).astype(np.int64)
    q[r.random_sample((2, Rcap)) < 0.5] = 0
    if Rcap >= 64:
        q[0, 3:40] = 0                                     # a long run of zeros
        q[1, :17] = 0                                      # zeros at the front
        q[0, Rcap - 5:] = 0                                # and at the end of the filled part
    q[0, Rcap // 2] = ref.Q_MAX                            # one row at the cap
    q[1, 0 if Rcap == 1 else Rcap // 3] = max(1, int(q[1, 0 if Rcap == 1 else Rcap // 3]))
    filled = Rcap if Rcap == 1 else Rcap - 3
    assert all(q[h, :filled].sum() >= 1 for h in range(2))
    return q, filled


@pytest.mark.parametrize("n", [1, 48])
@pytest.mark.parametrize("Rcap", [1, 64, 65, 4099])
def test_draw_equals_the_numpy_draw(hip, Rcap, n):
    q, filled = draw_table(Rcap)
    r = np.random.RandomState(Rcap + n)
    u = r.randint(0, 1 << 62, (2, n), dtype=np.int64)
    totals = [int(q[h, :filled].sum()) for h in range(2)]
    for h in range(2):                                     # the edges of the modulus: 0, total - 1, total (wraps to 0), beyond
        special = [0, totals[h] - 1, totals[h], totals[h] + 1, (1 << 62) - 1]
        if n == 1:
            u[h, 0] = special[(Rcap + h) % 3]
        else:
            u[h, :len(special)] = special
    qd, ud = dev(q.astype(np.int32)), dev(u)
    idx = torch.full((2, n), -5, dtype=torch.int64, device="cuda")
    scratch = torch.full((4 * ((Rcap + 1023) // 1024) + 2,), -1, dtype=torch.int64, device="cuda")
    hip.check(hip.lib().cadre_sil_draw(qd.data_ptr(), Rcap, filled, ud.data_ptr(), n, idx.data_ptr(), scratch.data_ptr(), hip.stream()),
              "cadre_sil_draw")
    got = host(idx)
    for h in range(2):
        want = ref.draw(q[h], filled, u[h])
        assert np.array_equal(got[h], want), (h, got[h], want)
        assert np.all(q[h][got[h]] > 0) and got[h].max() < filled
    assert np.array_equal(host(qd), q.astype(np.int32))   # the table is read only


def test_draw_past_one_scan_chunk(hip):
    """Rcap = 2^18 + 7: 257 block sums, one more than the 256 a scan pass takes; sums past 2^32."""
    Rcap, n = (1 << 18) + 7, 48
    r = np.random.RandomState(3)
    q = r.randint(0, 1 << 24, (2, Rcap)).astype(np.int64)
    q[:, ::3] = 0
    u = r.randint(0, 1 << 62, (2, n), dtype=np.int64)
    u[0, 0], u[1, 0] = int(q[0].sum()) - 1, 0
    qd, ud = dev(q.astype(np.int32)), dev(u)
    idx = torch.full((2, n), -5, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(4 * ((Rcap + 1023) // 1024) + 2, dtype=torch.int64, device="cuda")
    hip.check(hip.lib().cadre_sil_draw(qd.data_ptr(), Rcap, Rcap, ud.data_ptr(), n, idx.data_ptr(), scratch.data_ptr(), hip.stream()),
              "cadre_sil_draw")
    got = host(idx)
    assert int(q[0].sum()) > 1 << 32
    for h in range(2):
        assert np.array_equal(got[h], ref.draw(q[h], Rcap, u[h])), h


# ----------------------------------------------------------------------------- 7. cadre_sil_scatter
@pytest.mark.parametrize("with_pos", [False, True])
def test_scatter_equals_the_numpy_statement(hip, with_pos):
    Rcap, B, B_ppo, n = 200, 40, 16, 24
    r = np.random.RandomState(11 + with_pos)
    q = r.randint(0, 1000, (2, Rcap)).astype(np.int64)
    idx = np.stack([r.permutation(Rcap)[:n] for _ in range(2)]).astype(np.int64)
    w = np.abs(r.standard_normal((2, B))).astype(F4)
    pos = np.stack([r.permutation(B) for _ in range(2)]).astype(np.int32)
    for h in range(2):                                     # a row drawn twice: two SIL rows with the same inputs hold the same w
        idx[h, 5] = idx[h, 2]
        at = (lambda j: pos[h, B_ppo + j]) if with_pos else (lambda j: B_ppo + j)
        w[h, at(5)] = w[h, at(2)]
        w[h, at(7)] = 0.0
    qd, wd, idd, pd = dev(q.astype(np.int32)), dev(w), dev(idx), dev(pos)
    hip.check(hip.lib().cadre_sil_scatter(qd.data_ptr(), Rcap, idd.data_ptr(), n, wd.data_ptr(), pd.data_ptr() if with_pos else None, B,
                                          B_ppo, ALPHA, EPS, hip.stream()), "cadre_sil_scatter")
    got = host(qd).astype(np.int64)
    for h in range(2):
        want = ref.scatter(q[h], idx[h], w[h], pos[h] if with_pos else None, B_ppo, ALPHA, EPS)
        touched = np.zeros(Rcap, bool)
        touched[idx[h]] = True
        assert np.array_equal(got[h][~touched], q[h][~touched])
        print("scatter pos %s head %d: max |q - statement| %d quanta" % (with_pos, h, int(np.abs(got[h] - want).max())))
        assert np.array_equal(got[h], want) and np.all(got[h][touched] >= 1)
    # with alpha = 1, prio_eps = 0 and dyadic weights the power is exact: the table equals the statement exactly
    w2 = (r.randint(0, 64, (2, B)) / 16.0).astype(F4)
    qd2, wd2 = dev(q.astype(np.int32)), dev(w2)
    idx2 = np.stack([r.permutation(Rcap)[:n] for _ in range(2)]).astype(np.int64)
    hip.check(hip.lib().cadre_sil_scatter(qd2.data_ptr(), Rcap, dev(idx2).data_ptr(), n, wd2.data_ptr(), pd.data_ptr() if with_pos else None,
                                          B, B_ppo, 1.0, 0.0, hip.stream()), "cadre_sil_scatter")
    for h in range(2):
        assert np.array_equal(host(qd2)[h].astype(np.int64), ref.scatter(q[h], idx2[h], w2[h], pos[h] if with_pos else None, B_ppo, 1.0, 0.0))


# ----------------------------------------------------------------------------- 8. end to end
T_E, MBN, N_ENV, M_BUF = 16, 2, 2, 2
BW = T_E // MBN


def e2e_cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, lr=3e-4)
    d.update(kw)
    return d


def section_rollouts(section):
    """Synthetic storages with true terminations inside the rollout on both heads (rows before them are closed)."""
    from tests.test_ppo_stats_gpu import storages
    out = []
    for w in range(N_ENV):
        pair = storages(T_E, MBN, 700 + 10 * section + w)
        for h, s in enumerate(pair):
            s.masks.fill_(1.0)
            s.masks[5 + w + h] = 0.0
            s.masks[12 + h] = 0.0
            s.rewards.mul_(3.0)                            # returns that beat the critic on many rows
        out.append(pair)
    return out


def make(tmp):
    from ppo_agent.models import Shared_grad_buffers
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp)
    return agent, Shared_grad_buffers(agent.model_dict, agent.device)


def run_sections(tmp, mode, sections=2, coeffs=(0.0, 0.0), hyper=False):
    """mode None: no buffer; "sil": a buffer, appended after each section.  Per section (losses, parameters, generator state, stats,
    C-ABI calls)."""
    from cadre_amd import hip as h
    from cadre_amd.selfimit import SelfImitationBuffer
    from ppo_agent.train import learner_section_multi
    agent, shared = make(tmp)
    lrn = agent.learner
    buf = None
    if hyper:
        lrn.set_device_hyper(True)
    if mode == "sil":
        buf = SelfImitationBuffer(agent, M_BUF, N_ENV, T_E, alpha=ALPHA, prio_eps=EPS, seed=3)
        lrn.set_loss("ppo+sil", sil_coeff=coeffs[0], sil_value_coeff=coeffs[1])
        lrn.set_loss("ppo")
    torch.manual_seed(77)
    out = []
    for e in range(sections):
        rollouts, dones = section_rollouts(e), [False, e == 1]
        st = {}
        n0 = h.N_CALLS
        losses = learner_section_multi(agent, rollouts, dones, e2e_cfg(), shared, stats=st, episode=e,
                                       **({} if buf is None else dict(sil=buf)))
        out.append((losses, agent.arena.params.clone(), torch.get_rng_state().clone(), st, h.N_CALLS - n0))
        if buf is not None:
            buf.append(rollouts, dones)
    torch.cuda.synchronize()
    return agent, buf, out


def test_empty_buffer_and_zero_coefficients_change_nothing(tmp_path):
    """(a) the first section, buffer empty: the parent's launch census, losses, parameters and generator state.  (b) coefficients 0: the
    arena after a section WITH SIL rows is bit-identical to the section without `sil` (the SIL gradients are exact zeros, the PPO rows'
    bits do not depend on their neighbours)."""
    agent, buf, with_b = run_sections(tmp_path / "a", "sil")
    _a0, _none, plain = run_sections(tmp_path / "b", None)
    assert with_b[0][0] == plain[0][0] and torch.equal(with_b[0][1], plain[0][1]) and with_b[0][4] == plain[0][4]
    assert with_b[0][3]["sil"] == dict(filled=0, steps=0) and "sil" not in plain[0][3]
    for e in range(2):
        assert torch.equal(with_b[e][2], plain[e][2]), e                  # the buffer never draws from the global generator
    assert buf.ready and with_b[1][3]["sil"]["steps"] == MBN and with_b[1][4] > plain[1][4]
    assert torch.equal(with_b[1][1], plain[1][1]) and with_b[1][0] == plain[1][0]
    assert ((N_ENV + 1) * BW, agent.arena.Z, agent.learner.S) in agent.learner._ws
    s = with_b[1][3]["sil"]
    print("section 1 sil stats: %s" % (s,))
    assert s["rows"] == (float(BW), float(BW)) and all(0.0 <= v <= 1.0 for v in s["positive_share"]) and min(s["w_max"]) > 0
    assert agent.learner.loss_mode == "ppo" and (buf.filled, buf.next) == (2, 0)


def test_step_gradient_against_autograd_and_priorities_follow(tmp_path, hip):
    """(c) one mixed step with both coefficients positive: every parameter's gradient within 2e-4 of its model's max |g| of float64
    autograd through the oracle's nets of the PPO loss on the workers' rows + the SIL term on the drawn rows (the bar of
    tests/test_demo_mix_gpu.py for its mixed step).  (d) after the step the drawn rows' priorities are the quantised sil_w of the step,
    every other priority is untouched."""
    from cadre_amd import synth
    from cadre_amd.selfimit import SelfImitationBuffer
    from oracle import ppo_ref
    agent, _shared = make(tmp_path)
    lrn, C = agent.learner, 4
    lrn.use_sorted = False
    buf = SelfImitationBuffer(agent, M_BUF, N_ENV, T_E, alpha=ALPHA, prio_eps=EPS, seed=5)
    old = section_rollouts(0)
    buf.append(old, [False, False])
    assert buf.ready and (buf.filled, buf.next) == (1, 1)
    P = T_E + 1
    # append: R, flags, q of the slot are the numpy statements
    for e_, pair in enumerate(old):
        lo = buf.base(0, e_)
        for hd, (s, big) in enumerate(zip(pair, (buf.steer, buf.throttle))):
            f = lambda t: host(t).reshape(-1)
            Rn, fn = ref.closed_scan(f(s.rewards), f(s.masks), f(s.time_limits), f(s.value_preds), np.float32(s.gamma), "drop")
            assert np.array_equal(host(buf.flags[hd, lo:lo + P]), fn) and np.array_equal(f(big.returns[lo:lo + T_E]), Rn)
            assert np.abs(host(buf.q[hd, lo:lo + P]).astype(np.int64) - ref.initial_priorities(Rn, fn, f(s.value_preds), ALPHA, EPS)).max() <= 1
            assert torch.equal(big.value_preds[lo:lo + P], s.value_preds) and torch.equal(buf.steer._obs[lo:lo + P], pair[0]._obs)
    live = section_rollouts(1)
    advs = []
    for pair in live:
        for s in pair:
            s.returns.copy_(s.value_preds + 0.5 * torch.randn(s.returns.shape, generator=torch.Generator().manual_seed(3)).cuda())
            advs.append(torch.randn(T_E, 1, generator=torch.Generator().manual_seed(len(advs))).cuda())
    r = np.random.RandomState(4)
    idx = [torch.from_numpy(r.permutation(T_E)[:BW].astype(np.int64)) for _ in range(2 * N_ENV)]
    batches = [(live[w][0], idx[2 * w], advs[2 * w], live[w][1], idx[2 * w + 1], advs[2 * w + 1]) for w in range(N_ENV)]
    lrn.set_loss("ppo+sil", sil_coeff=SC, sil_value_coeff=SVC)
    lrn.set_loss("ppo")
    q_before = buf.q.clone()
    entries = buf.entries(BW, 1, 0, 0)
    assert len(entries) == 1 and entries[0][1].is_cuda and entries[0][1].shape == (BW,)
    sil_idx = np.stack([host(entries[0][1]), host(entries[0][4])])
    from cadre_amd.selfimit import sil_words
    words = sil_words(5, 0, 1, 0, 0, BW, 1).numpy()
    for hd in range(2):
        assert np.array_equal(sil_idx[hd], ref.draw(host(q_before[hd]).astype(np.int64), buf.rows_filled(), words[hd]))
    srow = torch.zeros(2, FS, device="cuda")
    agent.update_policy_from_storages(batches, sil=entries, sil_stats_row=srow)
    B_ppo, B = N_ENV * BW, (N_ENV + 1) * BW
    assert lrn.loss_mode == "ppo" and lrn._sil_rows is None and not lrn.sorted_rows(B)
    w = lrn.workspace(B)
    assert w["row_kind"][:, :B_ppo].sum().item() == 0 and w["row_kind"][:, B_ppo:].sum().item() == 2 * BW
    sil_w = host(w["sil_w"])
    buf.after_step(B_ppo)
    torch.cuda.synchronize()
    # (d) the priorities
    q_after = host(buf.q).astype(np.int64)
    for hd in range(2):
        want = ref.scatter(host(q_before[hd]).astype(np.int64), sil_idx[hd], sil_w[hd], None, B_ppo, ALPHA, EPS)
        assert np.abs(q_after[hd] - want).max() <= 1
        untouched = np.ones(buf.R, bool)
        untouched[sil_idx[hd]] = False
        assert np.array_equal(q_after[hd][untouched], host(q_before[hd]).astype(np.int64)[untouched])
        assert np.all(sil_w[hd, :B_ppo] == 0) and float(srow[hd, 5]) == BW
    # (c) the gradient
    params = {m: {k: p.double().requires_grad_(True) for k, p in d.items()} for m, d in ppo_ref.to_torch_params(synth.ppo_state(11)).items()}
    f2 = lambda t: host(t).reshape(t.shape[0], -1)
    cols = {k: np.zeros((2, B), np.float64) for k in ("act", "cmd", "ov", "ret", "olp", "adv")}
    kind = torch.zeros(2, B, dtype=torch.int32)
    kind[:, B_ppo:] = 1
    xs, h0s, c0s = [], [], []
    for hd in range(2):
        xo, hh, cc_ = [], [], []
        srcs = [(live[wk][hd], idx[2 * wk + hd].numpy(), advs[2 * wk + hd]) for wk in range(N_ENV)]
        big = (buf.steer, buf.throttle)[hd]
        srcs.append((big, sil_idx[hd], big.advantages))
        for k_, (s, t, adv) in enumerate(srcs):
            sl = slice(k_ * BW, (k_ + 1) * BW)
            for k, src in (("act", s.action), ("cmd", s.command), ("ov", s.value_preds), ("ret", s.returns), ("olp", s.action_log_probs),
                           ("adv", adv)):
                cols[k][hd, sl] = f2(src)[t, 0]
            xo.append(host(s._obs)[t][:, :, :530]); hh.append(host(s._hn)[t][:, :530]); cc_.append(host(s._cn)[t][:, :530])
        xs.append(np.concatenate(xo)); h0s.append(np.concatenate(hh)); c0s.append(np.concatenate(cc_))
    lg_rows, v_rows = [], []
    for hd, (head, K) in enumerate((("steer", 33), ("throttle", 3))):
        x = torch.from_numpy(xs[hd]).double().permute(1, 0, 2).reshape(-1, 530)        # time-major [S * B, 530]
        hid = (torch.from_numpy(h0s[hd]).double(), torch.from_numpy(c0s[hd]).double())
        for c in range(C):
            hh_, _ = ppo_ref.lstm_forward(x, hid, params["%s_lstm_%d" % (head, c)])
            lg_rows.append(torch.nn.functional.pad(ppo_ref.mlp3(hh_, params["%s_ppo_%d" % (head, c)], "control.linear"), (0, 64 - K)))
            v_rows.append(ppo_ref.mlp3(hh_, params["%s_ppo_%d" % (head, c)], "critic").view(-1))
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    lgs, vs = torch.stack(lg_rows), torch.stack(v_rows)
    cmd = tt(cols["cmd"], torch.int64)
    ppo = demo_mix_ref.ppo_rows_loss(lgs, vs, tt(cols["act"], torch.int64), cmd, tt(cols["ov"], torch.float64), tt(cols["ret"], torch.float64),
                                     tt(cols["olp"], torch.float64), tt(cols["adv"], torch.float64), kind, (33, 3), (None, None), C, lrn.clip,
                                     lrn.vc, lrn.cc, lrn.ec, 1.0 / BW)
    total, want_sil = ppo[3], []
    for hd, K in enumerate((33, 3)):
        rows = torch.arange(B_ppo, B)
        t_, pol, val = ref.sil_loss_torch(lgs[hd * C + cmd[hd, rows], rows, :K], vs[hd * C + cmd[hd, rows], rows],
                                          tt(cols["act"][hd, B_ppo:], torch.int64), tt(cols["ret"][hd, B_ppo:], torch.float64), SC, SVC)
        total = total + t_
        want_sil.append((float(pol.detach()), float(val.detach())))
        w64 = np.maximum(cols["ret"][hd, B_ppo:] - vs[hd * C + cmd[hd, rows], rows].detach().numpy(), 0)
        assert np.abs(sil_w[hd, B_ppo:] - w64).max() < 1e-4 and (w64 > 0).any()
    total.backward()
    worst = 0.0
    for mn, dct in params.items():
        gv = agent.arena.views(agent.arena.grads, mn)
        scale = max(float(p.grad.abs().max()) for p in dct.values() if p.grad is not None)
        for k, p in dct.items():
            g64 = torch.zeros_like(p) if p.grad is None else p.grad
            err = float((gv[k].cpu().double() - g64).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    got_sil = host(w["sil_losses"])
    print("mixed step with SIL rows: worst per-parameter error (rel. to model max |g|) %.2e; sil losses %s" % (worst, got_sil.tolist()))
    assert abs(got_sil[0] - sum(p for p, _v in want_sil)) < 1e-4 and abs(got_sil[1] - sum(v for _p, v in want_sil)) < 1e-4
    # sizes must agree
    with pytest.raises(ValueError, match="same"):
        agent.update_policy_from_storages(batches, sil=[(buf.steer, entries[0][1][:BW - 1], buf.steer.advantages, buf.throttle,
                                                         entries[0][4][:BW - 1], buf.throttle.advantages)])
    assert lrn.loss_mode == "ppo"


def test_device_hyper_mode_follows_the_block_without_a_new_graph(tmp_path):
    """(e) after set_hyper(sil_coeff = 2 x) the replayed graph writes exactly twice the SIL rows' dlogits (a power of two), the PPO
    rows' and every critic gradient stay, and no graph is added."""
    from cadre_amd.selfimit import SelfImitationBuffer
    agent, _shared = make(tmp_path)
    lrn = agent.learner
    buf = SelfImitationBuffer(agent, M_BUF, N_ENV, T_E, alpha=ALPHA, prio_eps=EPS, seed=5)
    buf.append(section_rollouts(0), [False, False])
    live = section_rollouts(1)
    idx = torch.arange(BW)
    batches = [(s, idx, s.advantages, t, idx, t.advantages) for s, t in live]
    lrn.set_device_hyper(True)
    lrn.set_hyper(sil_coeff=0.5, sil_value_coeff=0.25)
    entries = buf.entries(BW, 0, 0, 0)                      # (no after_step: the same rows every time)
    for _ in range(3):
        agent.update_policy_from_storages(batches, sil=entries)
    B_ppo, B = N_ENV * BW, (N_ENV + 1) * BW
    w = lrn.workspace(B)
    n_graphs = len(lrn._graphs)
    assert any(k[0] == "all" and ("sil", B_ppo) in k and ("hp",) in k for k in lrn._graphs if k[0] != "warm")
    before, sl_before = w["dO3"].clone(), w["sil_losses"].clone()
    lrn.set_hyper(sil_coeff=1.0)
    agent.update_policy_from_storages(batches, sil=entries)
    assert len(lrn._graphs) == n_graphs and lrn.hyper("sil_coeff") == 1.0 and lrn.hyper("sil_value_coeff") == 0.25
    after, C = w["dO3"], agent.arena.C
    for hd in range(2):
        act_b, act_a = before[2 * hd * C:2 * (hd + 1) * C:2], after[2 * hd * C:2 * (hd + 1) * C:2]
        crit_b, crit_a = before[2 * hd * C + 1:2 * (hd + 1) * C:2], after[2 * hd * C + 1:2 * (hd + 1) * C:2]
        assert torch.equal(act_a[:, B_ppo:], 2.0 * act_b[:, B_ppo:]) and float(act_b[:, B_ppo:].abs().max()) > 0
        assert torch.equal(act_a[:, :B_ppo], act_b[:, :B_ppo]) and torch.equal(crit_a, crit_b) and float(crit_b[:, B_ppo:].abs().max()) > 0
    assert float(w["sil_losses"][0]) == 2.0 * float(sl_before[0]) and float(w["sil_losses"][1]) == float(sl_before[1])
    assert lrn.loss_mode == "ppo"


def test_single_environment_section_takes_the_buffer(tmp_path):
    """learner_section (one environment) with `sil`: the first section is the plain one, the second carries SIL rows in every step and
    writes their priorities back; the loss mode is "ppo" again and the refused combinations raise."""
    from cadre_amd.selfimit import SelfImitationBuffer
    from ppo_agent.train import learner_section
    agent, shared = make(tmp_path)
    buf = SelfImitationBuffer(agent, M_BUF, 1, T_E, alpha=ALPHA, prio_eps=EPS, seed=9)
    agent.learner.set_loss("ppo+sil", sil_coeff=SC, sil_value_coeff=SVC)
    agent.learner.set_loss("ppo")
    seen = []
    for e in range(2):
        (s, t), st = section_rollouts(e)[0], {}
        q0 = buf.q.clone()
        vl, pl, el = learner_section(agent, s, t, False, e2e_cfg(), shared, stats=st, sil=buf, episode=e)
        assert len(vl) == MBN and all(np.isfinite(v) for v in vl + pl + el) and agent.learner.loss_mode == "ppo"
        seen.append((st["sil"], int((buf.q != q0).sum())))
        buf.append([(s, t)], [False])
    assert seen[0][0] == dict(filled=0, steps=0) and seen[0][1] == 0
    assert seen[1][0]["steps"] == MBN and seen[1][0]["rows"] == (float(BW), float(BW)) and seen[1][1] > 0
    (s, t) = section_rollouts(2)[0]
    with pytest.raises(ValueError, match="sil excludes"):
        learner_section(agent, s, t, False, e2e_cfg(), shared, sil=buf, demo=object())
    with pytest.raises(ValueError, match="fused_gather"):
        learner_section(agent, s, t, False, e2e_cfg(), shared, sil=buf, fused_gather=False)
    assert agent.learner.loss_mode == "ppo"


def test_train_vec_with_a_self_imitation_key(tmp_path):
    """(f) two episodes of train_vec with the key: the loss mode is "ppo" again afterwards, stats["sil"] is in the log line, the
    coefficient schedule is in the block; the key absent and the key None are the same run."""
    import types
    from cadre_amd import hip as h
    from ppo_agent import train as train_mod
    from tests.helpers import SyntheticEnv, topology_cfgs

    def run(tag, **extra):
        lines = []
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / tag), T=8, episodes=2)
        train_cfg.update(save_interval=10 ** 6, **extra)
        os.makedirs(str(tmp_path / tag), exist_ok=True)
        agent = train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=SyntheticEnv,
                                    logger=types.SimpleNamespace(log=lines.append))
        torch.cuda.synchronize()
        return agent, lines
    absent, _l = run("a", log_stats=True)
    none, plain_lines = run("b", log_stats=True, self_imitation=None)
    assert torch.equal(absent.arena.params, none.arena.params) and not none.learner.device_hyper
    agent, lines = run("c", log_stats=True, self_imitation=dict(rollouts=2, coeff=("linear", 1.0, 0.0), value_coeff=0.05,
                                                                 tail="bootstrap"))
    lrn = agent.learner
    stat_lines = [s for s in lines if "approx kl" in s]
    assert len(stat_lines) == 2 and "sil: 0 rollouts" in stat_lines[0] and "sil: 1 rollouts, w: " in stat_lines[1]
    assert not any("sil:" in s for s in plain_lines)
    assert lrn.loss_mode == "ppo" and lrn.device_hyper
    assert float(lrn._hp[h.HP_SIL_COEFF]) == 0.5 and float(lrn._hp[h.HP_SIL_VALUE_COEFF]) == 0.05
    assert agent.arena.step == absent.arena.step and bool(torch.isfinite(agent.arena.params).all())
    assert not torch.equal(agent.arena.params, absent.arena.params)
    with pytest.raises(ValueError, match="not part of a checkpoint"):
        run("d", self_imitation=dict(rollouts=2, coeff=0.1), checkpoint_interval=2)
    with pytest.raises(ValueError, match="sample_reuse"):
        run("e", self_imitation=dict(rollouts=2, coeff=0.1), sample_reuse=dict(rollouts=2))
