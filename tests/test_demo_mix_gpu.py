"""GPU: the demonstration term inside the PPO step — cadre_ppo_demo_loss row by row against the two kernels it extends (bit
for bit), its sums against float64 autograd (tests/demo_mix_ref.py), cadre_mix_row_kinds, the whole mixed step against the
existing PPO and imitation steps (gradient linearity), device-hyper mode, the mode switched off, a learning check and
train_vec with train_cfg["demo_mix"]."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import demo_mix_ref, imitation_ref, ordinal_ref
from tests.test_imitation_gpu import make_agent, random_demo, record_episodes, rel, steer_rank

pytestmark = pytest.mark.gpu
CLIP, VC, CC, EC = 0.1, 0.1, 1.0, 0.01
EPS, DC, DVC = 0.1, 0.7, 0.3
NS, NT = 33, 3
FP, FD = 8, imitation_ref.BC_STATS_FIELDS
# (B, B_ppo, C): a workgroup of 16 rows holds both kinds, the last workgroup is part-filled (24, 40), and B = 64 is where the
# row-sorted layout of the update switches on
CASES = [(24, 12, 3), (40, 24, 4), (64, 32, 4)]


def ord_table(ranks):
    t = torch.zeros(2, 64, dtype=torch.int32)
    for h, r in enumerate(ranks):
        if r is None:
            t[h, 0] = -1
        else:
            t[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return t.cuda()


@functools.lru_cache(maxsize=None)
def mix_case(B, B_ppo, C, layout="prefix"):
    """Inputs (ldl = 64, finite logits) shared by every variant of a case.  layout: "prefix" — rows B_ppo .. B - 1 are the
    demonstration rows; "random" — B - B_ppo demonstration rows at random positions, other positions per head.  Old
    log-probs sit around the row's own categorical log-prob (ratios on both sides of the clip).  In every case, per head:
    a PPO row with command -1 and one with command C, a demonstration row with each, and a demonstration row with action -1."""
    g = torch.Generator().manual_seed(1000 * B + B_ppo + (17 if layout == "random" else 0))
    K = (NS, NT)
    logits = torch.zeros(2 * C, B, 64)
    logits[:C, :, :NS] = torch.randn(C, B, NS, generator=g)
    logits[C:, :, :NT] = torch.randn(C, B, NT, generator=g)
    values = torch.randn(2 * C, B, generator=g)
    actions = torch.stack([torch.randint(0, NS, (B,), generator=g), torch.randint(0, NT, (B,), generator=g)])
    cmds = torch.randint(0, C, (2, B), generator=g, dtype=torch.int32)
    old_v, rets, adv = (torch.randn(2, B, generator=g) for _ in range(3))
    old_lp = torch.zeros(2, B)
    for hd in range(2):
        own = logits[hd * C + cmds[hd].long(), torch.arange(B), :K[hd]]
        lp = ordinal_ref.normalised_logits(own, None).gather(1, actions[hd].view(-1, 1)).view(-1).float()
        old_lp[hd] = lp + 0.3 * torch.randn(B, generator=g)
    kind = torch.zeros(2, B, dtype=torch.int32)
    for hd in range(2):
        if layout == "prefix":
            kind[hd, B_ppo:] = 1
        else:
            kind[hd, torch.randperm(B, generator=g)[:B - B_ppo]] = 1
    adv = torch.where(kind == 0, adv, torch.rand(2, B, generator=g) * 3.75 + 0.25)    # demonstration rows: the row weight
    for hd in range(2):
        p, d = torch.nonzero(kind[hd] == 0).view(-1), torch.nonzero(kind[hd] == 1).view(-1)
        if p.numel() >= 3:
            cmds[hd, p[0]], cmds[hd, p[1]] = -1, C
        if d.numel() >= 4:
            cmds[hd, d[0]], cmds[hd, d[1]] = -1, C
            actions[hd, d[2]] = -1
    ranks = (steer_rank(NS, g), torch.randperm(NT, generator=g).tolist())
    return dict(logits=logits, values=values, actions=actions, cmds=cmds, old_v=old_v, rets=rets, old_lp=old_lp, adv=adv,
                kind=kind), ranks


def scales(B, B_ppo):
    return 1.0 / max(B_ppo, 1), 1.0 / max(B - B_ppo, 1)


@functools.lru_cache(maxsize=None)
def mix_ref(B, B_ppo, C, layout, ordinal):
    """float64: (losses[3], demo_losses[2], d total / d raw, d total / d value, stats [2][6], demo stats [2][6]), once."""
    inp, ranks = mix_case(B, B_ppo, C, layout)
    inv_b, inv_bd = scales(B, B_ppo)
    lg, vv = inp["logits"].double().requires_grad_(True), inp["values"].double().requires_grad_(True)
    out = demo_mix_ref.mixed_loss(lg, vv, inp["actions"], inp["cmds"], inp["old_v"], inp["rets"], inp["old_lp"], inp["adv"],
                                  inp["kind"], (NS, NT), ranks if ordinal else (None, None), C, CLIP, VC, CC, EC, inv_b, EPS, DC,
                                  DVC, inv_bd)
    out["total"].backward()
    f = lambda ts: torch.tensor([float(torch.as_tensor(t).detach()) for t in ts])
    return f(out["losses"]), f(out["demo_losses"]), lg.grad, vv.grad, out["stats"], out["demo_stats"]


def dev_inputs(inp, **over):
    d = {k: v.cuda() for k, v in inp.items()}
    d.update({k: v.cuda() for k, v in over.items()})
    return d


def hp_block(**over):
    from cadre_amd import hip
    hp = torch.zeros(hip.HP_FIELDS, dtype=torch.float64)
    hp[hip.HP["lr"]], hp[hip.HP["clip"]], hp[hip.HP["value_coeff"]] = 3e-4, CLIP, VC
    hp[hip.HP["clip_coeff"]], hp[hip.HP["ent_coeff"]], hp[hip.HP["max_grad_norm"]] = CC, EC, 250.0
    hp[hip.HP_DEMO_COEFF], hp[hip.HP_DEMO_VALUE_COEFF] = DC, DVC
    for k, v in over.items():
        hp[hip.HP_INDEX[k]] = v
    return hp.cuda()


def new_outputs(B, C):
    nblk = (B + 15) // 16
    out = dict(losses=torch.full((3,), 7.0, device="cuda"), demo_losses=torch.full((2,), 7.0, device="cuda"),
               dl=torch.full((2 * C, B, 64), 9.0, device="cuda"), dv=torch.full((2 * C, B), 9.0, device="cuda"),
               scratch=torch.full((4 + 6 * nblk,), 3.0, device="cuda"),
               demo_scratch=torch.full((2 * nblk * (2 + FD),), 3.0, device="cuda"),             # needs no initialisation
               stats=torch.full((2, FP), 5.0, device="cuda"), sscr=torch.full((12 * nblk,), 3.0, device="cuda"),
               demo_stats=torch.full((2, FD), 5.0, device="cuda"), bscr=torch.full((2 * nblk * FD,), 3.0, device="cuda"),
               stop=torch.zeros(1, dtype=torch.int32, device="cuda"))
    out["scratch"][0] = 0.0                                # the arrival counter: zero on first use, reset by every launch
    return out


def head_args(d, B, C):
    return (d["logits"].data_ptr(), 64, B * 64, d["values"].data_ptr(), 1, B, d["actions"].data_ptr(), d["cmds"].data_ptr())


def run_mix(d, o, B, C, table, inv_b, inv_bd, hp=None, stats=False, dstats=True, target_kl=0.0, coeffs=(DC, DVC), eps=EPS):
    from cadre_amd import hip
    hip.check(hip.lib().cadre_ppo_demo_loss(
        *head_args(d, B, C), d["old_v"].data_ptr(), d["rets"].data_ptr(), d["old_lp"].data_ptr(), d["adv"].data_ptr(),
        d["kind"].data_ptr(), B, C, NS, NT, None if hp is None else hp.data_ptr(), CLIP, VC, CC, EC, inv_b, eps, coeffs[0],
        coeffs[1], inv_bd, o["losses"].data_ptr(), o["demo_losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(),
        o["scratch"].data_ptr(), o["demo_scratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None, FP,
        o["sscr"].data_ptr() if stats else None, target_kl, o["stop"].data_ptr() if stats else None,
        o["demo_stats"].data_ptr() if dstats else None, FD, None if table is None else table.data_ptr(), hip.stream()),
        "cadre_ppo_demo_loss")
    assert float(o["scratch"][0]) == 0.0                   # the counter is left zero
    return o


def run_ppo(d, o, B, C, table, inv_b, hp=None, stats=False, target_kl=0.0):
    from cadre_amd import hip
    hip.check(hip.lib().cadre_ppo_loss_ord(
        *head_args(d, B, C), d["old_v"].data_ptr(), d["rets"].data_ptr(), d["old_lp"].data_ptr(), d["adv"].data_ptr(), B, C,
        NS, NT, None if hp is None else hp.data_ptr(), CLIP, VC, CC, EC, inv_b, o["losses"].data_ptr(), o["dl"].data_ptr(),
        o["dv"].data_ptr(), o["scratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None, FP,
        o["sscr"].data_ptr() if stats else None, target_kl, o["stop"].data_ptr() if stats else None, table.data_ptr(),
        hip.stream()), "cadre_ppo_loss_ord")
    return o


def run_bc(d, o, B, C, table, inv_b):
    """cadre_bc_loss with bc_coeff = demo_coeff, value_coeff = demo_value_coeff, ent_coeff = 0, the weights from `adv`."""
    from cadre_amd import hip
    hip.check(hip.lib().cadre_bc_loss(
        *head_args(d, B, C), d["rets"].data_ptr(), d["adv"].data_ptr(), B, C, NS, NT, EPS, DC, DVC, 0.0, inv_b,
        o["losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(), None, o["demo_stats"].data_ptr(),
        FD, o["bscr"].data_ptr(), table.data_ptr(), hip.stream()), "cadre_bc_loss")
    return o


def table_of(ranks, ordinal):
    return ord_table(ranks if ordinal else (None, None))


def head_rows(t, hd, C, rows):
    return t[hd * C:(hd + 1) * C][:, rows]


# ----------------------------------------------------------------------------- 1. per-row bit equality
@pytest.mark.parametrize("layout", ["prefix", "random"])
@pytest.mark.parametrize("ordinal", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_rows_are_the_two_parent_kernels_bit_for_bit(case, ordinal, layout):
    """Every PPO row's dlogits (all ldl columns, all C nets) and dvalues equal what cadre_ppo_loss_ord writes for that row
    on the same inputs, every demonstration row's what cadre_bc_loss writes (bc_coeff = demo_coeff, value_coeff =
    demo_value_coeff, ent_coeff = 0, inv_b = inv_bd), by value and with the device hyper-parameter block: torch.equal, no
    tolerance.  Three repeated launches on one scratch give the same bits."""
    B, B_ppo, C = case
    inp, ranks = mix_case(B, B_ppo, C, layout)
    inv_b, inv_bd = scales(B, B_ppo)
    d, table = dev_inputs(inp), table_of(ranks, ordinal)
    mix = run_mix(d, new_outputs(B, C), B, C, table, inv_b, inv_bd)
    mix_hp = run_mix(d, new_outputs(B, C), B, C, table, inv_b, inv_bd, hp=hp_block(), coeffs=(0.0, 0.0))
    mix_st = run_mix(d, new_outputs(B, C), B, C, table, inv_b, inv_bd, hp=hp_block(), stats=True, coeffs=(0.0, 0.0))
    ppo = run_ppo(d, new_outputs(B, C), B, C, table, inv_b)
    ppo_hp = run_ppo(d, new_outputs(B, C), B, C, table, inv_b, hp=hp_block())
    bc = run_bc(d, new_outputs(B, C), B, C, table, inv_bd)
    assert bool(torch.isfinite(mix["dl"]).all()) and bool(torch.isfinite(mix["dv"]).all())
    for other in (mix_hp, mix_st):
        assert all(torch.equal(other[k], mix[k]) for k in ("losses", "demo_losses", "dl", "dv", "demo_stats"))
    for hd in range(2):
        p = torch.nonzero(d["kind"][hd] == 0).view(-1)
        q = torch.nonzero(d["kind"][hd] != 0).view(-1)
        for want in (ppo, ppo_hp):
            assert torch.equal(head_rows(mix["dl"], hd, C, p), head_rows(want["dl"], hd, C, p))
            assert torch.equal(head_rows(mix["dv"], hd, C, p), head_rows(want["dv"], hd, C, p))
        assert torch.equal(head_rows(mix["dl"], hd, C, q), head_rows(bc["dl"], hd, C, q))
        assert torch.equal(head_rows(mix["dv"], hd, C, q), head_rows(bc["dv"], hd, C, q))
        assert float(head_rows(mix["dl"], hd, C, p).abs().max()) > 0 and float(head_rows(mix["dl"], hd, C, q).abs().max()) > 0
        # the marked rows: a demonstration row with a bad command or no label gets exact zeros in all C nets
        cq, aq = d["cmds"][hd][q], d["actions"][hd][q]
        out = q[(cq < 0) | (cq >= C) | (aq < 0)]
        assert out.numel() == 3 and float(head_rows(mix["dl"], hd, C, out).abs().max()) == 0.0
        assert float(head_rows(mix["dv"], hd, C, out).abs().max()) == 0.0
    first = {k: mix[k].clone() for k in ("losses", "demo_losses", "dl", "dv", "demo_stats")}
    for _ in range(3):
        run_mix(d, mix, B, C, table, inv_b, inv_bd)
        assert all(torch.equal(mix[k], first[k]) for k in first)


# ----------------------------------------------------------------------------- 2. degenerate launches
@pytest.mark.parametrize("ordinal", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_all_ppo_rows_is_the_ppo_kernel(case, ordinal):
    """B_ppo = B: losses, the PPO stats row, the stop flag and the block's lr after the KL-adaptive rule are bit-identical
    to cadre_ppo_loss_ord on the same inputs (a gate that fires: lr stays; one that does not: lr moves); demo_losses = 0."""
    from cadre_amd import hip
    B, _bp, C = case
    inp, ranks = mix_case(B, _bp, C)
    # (every row is a PPO row here: the unlabelled demonstration rows of the case get a bin)
    d = dev_inputs(inp, kind=torch.zeros(2, B, dtype=torch.int32), actions=inp["actions"].clamp(min=0))
    table = table_of(ranks, ordinal)
    for tkl in (1e-6, 1e3):
        hp_m, hp_p = (hp_block(desired_kl=1e-5, lr_min=1e-5, lr_max=1e-2, lr_factor=1.5) for _ in range(2))
        mix = run_mix(d, new_outputs(B, C), B, C, table, 1.0 / B, 1.0, hp=hp_m, stats=True, target_kl=tkl)
        ppo = run_ppo(d, new_outputs(B, C), B, C, table, 1.0 / B, hp=hp_p, stats=True, target_kl=tkl)
        assert all(torch.equal(mix[k], ppo[k]) for k in ("losses", "dl", "dv", "stop")) and torch.equal(hp_m, hp_p)
        assert torch.equal(mix["stats"][:, :7], ppo["stats"][:, :7])            # (field 7 belongs to cadre_grad_norms_hp)
        assert int(mix["stop"]) == (1 if tkl < 1 else 0) and float(mix["stats"][0, 6]) == (0.0 if tkl < 1 else 1.0)
        assert (float(hp_m[hip.HP["lr"]]) == 3e-4) == (tkl < 1)
        assert float(mix["demo_losses"].abs().max()) == 0.0 and float(mix["demo_stats"].abs().max()) == 0.0
    plain = run_mix(d, new_outputs(B, C), B, C, table, 1.0 / B, 1.0)
    want = run_ppo(d, new_outputs(B, C), B, C, table, 1.0 / B)
    assert all(torch.equal(plain[k], want[k]) for k in ("losses", "dl", "dv")) and float((plain["stats"] - 5.0).abs().max()) == 0.0


@pytest.mark.parametrize("ordinal", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_all_demonstration_rows_is_the_imitation_kernel(case, ordinal):
    """B_ppo = 0: demo_losses and the demo stats row are bit-identical to cadre_bc_loss's losses[1], losses[0] and stats
    with the scalars of the row test; losses = 0; three repeated launches on one scratch give the same bits."""
    B, _bp, C = case
    inp, ranks = mix_case(B, _bp, C)
    d, table = dev_inputs(inp, kind=torch.ones(2, B, dtype=torch.int32)), table_of(ranks, ordinal)
    mix = run_mix(d, new_outputs(B, C), B, C, table, 1.0, 1.0 / B, stats=True)
    bc = run_bc(d, new_outputs(B, C), B, C, table, 1.0 / B)
    assert torch.equal(mix["demo_losses"], torch.stack([bc["losses"][1], bc["losses"][0]])) and float(bc["losses"][2]) == 0.0
    assert torch.equal(mix["demo_stats"], bc["demo_stats"]) and torch.equal(mix["dl"], bc["dl"]) and torch.equal(mix["dv"], bc["dv"])
    assert float(mix["losses"].abs().max()) == 0.0 and float(mix["stats"][:, :6].abs().max()) == 0.0
    assert float(mix["demo_losses"][0]) > 0 and int(mix["stop"]) == 0
    first = {k: mix[k].clone() for k in ("losses", "demo_losses", "dl", "dv", "demo_stats", "stats")}
    for _ in range(3):
        run_mix(d, mix, B, C, table, 1.0, 1.0 / B, stats=True)
        assert all(torch.equal(mix[k], first[k]) for k in first)


# ----------------------------------------------------------------------------- 3. sums against float64
@pytest.mark.parametrize("layout", ["prefix", "random"])
@pytest.mark.parametrize("ordinal", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_sums_against_float64(case, ordinal, layout):
    """losses, demo_losses and dvalues within 1e-5, dlogits within 2e-5 of the largest reference magnitude, both stats rows
    within 1e-5 absolute, accuracy / clip-fraction / row counts exact: the bars tests/test_imitation_gpu.py and
    tests/test_ordinal_gpu.py hold the two parent kernels to, for the same statements."""
    B, B_ppo, C = case
    inp, ranks = mix_case(B, B_ppo, C, layout)
    inv_b, inv_bd = scales(B, B_ppo)
    want_l, want_d, want_dl, want_dv, want_st, want_ds = mix_ref(B, B_ppo, C, layout, ordinal)
    o = run_mix(dev_inputs(inp), new_outputs(B, C), B, C, table_of(ranks, ordinal), inv_b, inv_bd, stats=True)
    e_l, e_d, e_dv, e_dl = rel(o["losses"], want_l), rel(o["demo_losses"], want_d), rel(o["dv"], want_dv), rel(o["dl"], want_dl)
    e_st = float((o["stats"][:, :6].double().cpu() - want_st).abs().max())
    e_ds = float((o["demo_stats"].double().cpu() - want_ds).abs().max())
    print("case %s ordinal %s %s: losses %.2e demo losses %.2e dvalues %.2e dlogits %.2e stats %.2e demo stats %.2e"
          % (case, ordinal, layout, e_l, e_d, e_dv, e_dl, e_st, e_ds))
    assert e_l < 1e-5 and e_d < 1e-5 and e_dv < 1e-5 and e_dl < 2e-5, (e_l, e_d, e_dv, e_dl)
    assert e_st < 1e-5 and e_ds < 1e-5, (e_st, e_ds)
    for k in (2, 3):                                       # clip fractions: exact counts
        assert torch.equal((o["stats"][:, k].double().cpu() / inv_b).round(), (want_st[:, k] / inv_b).round())
    for k in (0, 5):                                       # accuracy, rows counted
        assert torch.equal((o["demo_stats"][:, k].double().cpu() / inv_bd).round(), (want_ds[:, k] / inv_bd).round())
    assert float(o["stats"][0, 6]) == 1.0 and float(o["stats"][1, 6]) == 1.0
    assert float(o["dl"][:C, :, NS:].abs().max()) == 0.0 and float(o["dl"][C:, :, NT:].abs().max()) == 0.0


def test_kl_gate_sees_the_ppo_rows_only():
    """Demonstration rows whose old_logp slot would give a huge KL if read: the PPO stats and the stop flag are those of the
    PPO rows alone (the float64 reference; bit for bit a launch with harmless values in those slots), and target_kl just
    above / below the PPO rows' KL flips `applied`."""
    B, B_ppo, C = 40, 24, 4
    inp, ranks = mix_case(B, B_ppo, C, "random")
    inv_b, inv_bd = scales(B, B_ppo)
    _l, _d, _dl, _dv, want_st, _ds = mix_ref(B, B_ppo, C, "random", False)
    bad_lp = torch.where(inp["kind"] == 0, inp["old_lp"], torch.full_like(inp["old_lp"], -1000.0))
    bad_ov = torch.where(inp["kind"] == 0, inp["old_v"], torch.full_like(inp["old_v"], 1e30))
    table = table_of(ranks, False)
    good = run_mix(dev_inputs(inp), new_outputs(B, C), B, C, table, inv_b, inv_bd, stats=True, target_kl=1e3)
    bad = run_mix(dev_inputs(inp, old_lp=bad_lp, old_v=bad_ov), new_outputs(B, C), B, C, table, inv_b, inv_bd, stats=True,
                  target_kl=1e3)
    assert all(torch.equal(bad[k], good[k]) for k in ("losses", "demo_losses", "dl", "dv", "stats", "demo_stats", "stop"))
    assert float((bad["stats"][:, :6].double().cpu() - want_st).abs().max()) < 1e-5 and int(bad["stop"]) == 0
    kl = float(want_st[:, 0].max())
    assert kl > 1e-3
    for factor, applied in ((0.99, 0.0), (1.01, 1.0)):     # the gate: max KL > 1.5 target_kl
        o = run_mix(dev_inputs(inp, old_lp=bad_lp), new_outputs(B, C), B, C, table, inv_b, inv_bd, stats=True,
                    target_kl=factor * kl / 1.5)
        assert float(o["stats"][0, 6]) == applied and float(o["stats"][1, 6]) == applied and int(o["stop"]) == 1 - int(applied)


# ----------------------------------------------------------------------------- 4. cadre_mix_row_kinds
@pytest.mark.parametrize("B,B_ppo", [(24, 12), (24, 0), (24, 24), (300, 77)])
def test_mix_row_kinds(B, B_ppo):
    from cadre_amd import hip
    L = hip.lib()
    r = np.random.RandomState(B + B_ppo)
    pos = np.stack([r.permutation(B), r.permutation(B)]).astype(np.int32)
    pos_d = torch.from_numpy(pos).cuda()
    for p, want_pos in ((None, np.stack([np.arange(B)] * 2)), (pos_d, pos)):
        kind = torch.full((2, B), 7, dtype=torch.int32, device="cuda")
        hip.check(L.cadre_mix_row_kinds(None if p is None else p.data_ptr(), B, B_ppo, kind.data_ptr(), hip.stream()),
                  "cadre_mix_row_kinds")
        want = np.zeros((2, B), np.int32)
        for hd in range(2):
            want[hd, want_pos[hd]] = (np.arange(B) >= B_ppo)
        assert np.array_equal(kind.cpu().numpy(), want)
    assert L.cadre_mix_row_kinds(None, B, B + 1, pos_d.data_ptr(), hip.stream()) == -1
    assert L.cadre_mix_row_kinds(None, B, -1, pos_d.data_ptr(), hip.stream()) == -1
    assert L.cadre_mix_row_kinds(None, B, B_ppo, None, hip.stream()) == -1


# ----------------------------------------------------------------------------- 5. the whole step
def ppo_storages(T, seed):
    """A steer / throttle storage pair of T random rows (no encoder) and their advantage tensors."""
    from ppo_agent.storage import RolloutStorage
    r = np.random.RandomState(seed)
    pair, advs = [], []
    for K in (NS, NT):
        st = RolloutStorage(T, 1, 530, 8, 530, True, 0.99, 0.95)
        st.to("cuda:0")
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        st.obs[:T].copy_(f((r.standard_normal((T, 8, 530)) * 0.5).astype(np.float32)))
        st.command[:T, 0].copy_(f(r.randint(0, 4, T).astype(np.int32)))
        st.action[:T, 0].copy_(f(r.randint(0, K, T).astype(np.int64)))
        st.value_preds[:T, 0].copy_(f((0.3 * r.standard_normal(T)).astype(np.float32)))
        st.returns[:T, 0].copy_(f(r.standard_normal(T).astype(np.float32)))
        st.action_log_probs[:T, 0].copy_(f((-np.log(K) + 0.2 * r.standard_normal(T)).astype(np.float32)))
        pair.append(st)
        advs.append(f(r.standard_normal((T, 1)).astype(np.float32)))
    return pair, advs


def model_grads(agent):
    g = agent.arena.grads.clone()
    return {m: {k: v.double() for k, v in agent.arena.views(g, m).items()} for m in agent.arena.model_names()}


@pytest.mark.parametrize("Bw,sort,placed", [(12, False, None), (32, True, True), (32, True, False)])
def test_mixed_step_is_the_sum_of_the_ppo_and_the_imitation_step(tmp_path, Bw, sort, placed):
    """Gradient linearity, the acceptance test: after update_policy_from_storages(batches, demo=entries) the gradients of
    every net equal (a) those of update_policy_from_storages(batches) plus (b) those of imitate_from_storages(entries) with
    bc_coeff = demo_coeff, ent_coeff = 0 and value_coeff = demo_value_coeff, within 2e-4 of each model's max |g| (only the
    order of fp32 row sums differs).  Unsorted B = 24; sorted B = 64 with the one-launch gather and through
    cadre_sort_rows_by_command + cadre_permute_minibatch.  Eager, warm-up and graph replay give the same bits."""
    agent = make_agent(tmp_path)
    lrn = agent.learner
    lrn.use_sorted = sort
    agent.gather_sorted = placed
    B = 2 * Bw
    assert lrn.sorted_rows(B) == sort
    (ps, pt), (adv_s, adv_t) = ppo_storages(32, seed=Bw)
    demo, _host = random_demo(agent, 40, seed=3)
    r = np.random.RandomState(4)
    idx_s, idx_t = (torch.from_numpy(r.permutation(32)[:Bw].astype(np.int64)) for _ in range(2))
    others = [int(x) for x in r.permutation(40) if x != 1][:Bw - 1]
    idx_d = torch.tensor([1] + others, dtype=torch.int64)                     # (row 1: the unlabelled steer row of random_demo)
    batches, entries = [(ps, idx_s, adv_s, pt, idx_t, adv_t)], demo.batch(idx_d)
    calls = []
    for _ in range(3):
        got = agent.update_policy_from_storages(batches, demo=entries, demo_label_smoothing=EPS, demo_coeff=DC,
                                                demo_value_coeff=DVC)
        w = lrn.workspace(B)
        calls.append((got, agent.arena.grads.clone(), w["demo_losses"].clone(), w["demo_stats"].clone()))
    assert lrn.loss_mode == "ppo" and lrn._demo_rows is None and lrn._mode_key() == ()      # restored on exit
    assert any(k[0] == "all" and ("demo", EPS, Bw, DC, DVC) in k for k in lrn._graphs if k[0] != "warm")
    for c in calls[1:]:
        assert c[0] == calls[0][0] and all(torch.equal(x, y) for x, y in zip(c[1:], calls[0][1:]))
    g_mix = model_grads(agent)
    l_a = agent.update_policy_from_storages(batches)
    g_a = model_grads(agent)
    vc, ec = lrn.vc, lrn.ec
    lrn.vc, lrn.ec = DVC, 0.0
    try:
        l_b = agent.imitate_from_storages(entries, label_smoothing=EPS, bc_coeff=DC)
    finally:
        lrn.vc, lrn.ec = vc, ec
    g_b = model_grads(agent)
    worst = 0.0
    for m in g_mix:
        scale = max(float((g_a[m][k] + g_b[m][k]).abs().max()) for k in g_mix[m])
        assert scale > 0
        for k in g_mix[m]:
            err = float((g_mix[m][k] - (g_a[m][k] + g_b[m][k])).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-4, (m, k, err)
    e_l = max(abs(x - y) for x, y in zip(calls[0][0], l_a))
    e_d = abs(float(calls[0][2][0]) - l_b[1])
    print("Bw %d sorted %s placed %s: worst gradient error %.2e of the model's max |g|; losses %.2e, demo loss %.2e"
          % (Bw, sort, placed, worst, e_l, e_d))
    assert e_l < 1e-5 and e_d < 1e-5 and abs(float(calls[0][2][1]) - l_b[0]) < 1e-5
    assert float(calls[0][3][0, 5]) == pytest.approx((Bw - 1) / Bw) and float(calls[0][3][1, 5]) == 1.0
    # a different geometry is not silently mixed: sizes must agree
    with pytest.raises(ValueError, match="same"):
        agent.update_policy_from_storages(batches, demo=demo.batch(idx_d[:Bw - 1]))
    assert lrn.loss_mode == "ppo"


# ----------------------------------------------------------------------------- 6. device-hyper mode
def test_device_hyper_mode_follows_the_block_without_a_new_graph(tmp_path):
    """After set_hyper(demo_coeff = 2 x) the replayed graph writes exactly twice the demonstration rows' dlogits (a power of
    two), the PPO rows' stay, and no graph is added."""
    agent = make_agent(tmp_path)
    lrn = agent.learner
    Bw, B = 12, 24
    (ps, pt), (adv_s, adv_t) = ppo_storages(32, seed=6)
    demo, _host = random_demo(agent, 40, seed=7)
    idx = torch.arange(Bw)
    batches, entries = [(ps, idx, adv_s, pt, idx, adv_t)], demo.batch(idx + 2)
    lrn.set_device_hyper(True)
    lrn.set_hyper(demo_coeff=0.5, demo_value_coeff=0.25)
    for _ in range(3):
        agent.update_policy_from_storages(batches, demo=entries)
    w = lrn.workspace(B)
    n_graphs = len(lrn._graphs)
    assert any(k[0] == "all" and ("demo", 0.0, Bw) in k and ("hp",) in k for k in lrn._graphs if k[0] != "warm")
    before, dl_before = w["dO3"].clone(), w["demo_losses"].clone()
    lrn.set_hyper(demo_coeff=1.0)
    agent.update_policy_from_storages(batches, demo=entries)
    assert len(lrn._graphs) == n_graphs and lrn.hyper("demo_coeff") == 1.0
    after, C = w["dO3"], agent.arena.C
    kind = w["row_kind"]
    assert kind[:, :Bw].sum().item() == 0 and kind[:, Bw:].sum().item() == 2 * Bw
    for hd in range(2):
        act_b, act_a = before[2 * hd * C:2 * (hd + 1) * C:2], after[2 * hd * C:2 * (hd + 1) * C:2]
        crit_b, crit_a = before[2 * hd * C + 1:2 * (hd + 1) * C:2], after[2 * hd * C + 1:2 * (hd + 1) * C:2]
        assert torch.equal(act_a[:, Bw:], 2.0 * act_b[:, Bw:]) and float(act_b[:, Bw:].abs().max()) > 0
        assert torch.equal(act_a[:, :Bw], act_b[:, :Bw]) and torch.equal(crit_a, crit_b) and float(crit_b[:, Bw:].abs().max()) > 0
    assert float(w["demo_losses"][0]) == 2.0 * float(dl_before[0]) and float(w["demo_losses"][1]) == float(dl_before[1])
    assert lrn.loss_mode == "ppo"


# ----------------------------------------------------------------------------- 7. mode off
def test_mode_off_changes_nothing(tmp_path):
    """demo=None: the launches of a step (hip.N_CALLS, learner.launches) and the workspace keys are what they are without
    the feature, before and after a mixed step ran on the same agent; the mixed step is one launch more (the row kinds)."""
    from cadre_amd import hip
    agent = make_agent(tmp_path)
    lrn = agent.learner
    lrn.use_graphs = False
    Bw = 12
    (ps, pt), (adv_s, adv_t) = ppo_storages(32, seed=8)
    demo, _host = random_demo(agent, 40, seed=9)
    idx = torch.arange(Bw)
    batches, entries = [(ps, idx, adv_s, pt, idx, adv_t)], demo.batch(idx)

    def calls(**kw):
        n0 = hip.N_CALLS
        out = agent.update_policy_from_storages(batches, **kw)
        return hip.N_CALLS - n0, out
    calls()                                                # (the first step of an agent also packs the recurrent weights)
    n_plain, l_plain = calls()
    g_plain = agent.arena.grads.clone()
    new_keys = {"row_kind", "demo_losses", "demo_stats", "demo_scratch"}
    assert not new_keys & set(lrn.workspace(Bw)) and lrn._mode_key() == ()
    n_none, l_none = calls(demo=None)
    assert n_none == n_plain and l_none == l_plain
    # the mixed step at the same B (one worker entry + one demonstration entry against two worker entries)
    n0 = hip.N_CALLS
    agent.update_policy_from_storages(batches + batches)
    n_two = hip.N_CALLS - n0
    n0 = hip.N_CALLS
    agent.update_policy_from_storages(batches, demo=entries, demo_coeff=DC)
    n_mix = hip.N_CALLS - n0
    assert n_mix == n_two + 1 and new_keys <= set(lrn.workspace(2 * Bw)) and not new_keys & set(lrn.workspace(Bw))
    n_again, l_again = calls()
    assert n_again == n_plain and l_again == l_plain and torch.equal(agent.arena.grads, g_plain)
    with pytest.raises(hip.CadreHipError, match="ppo\\+demo"):
        lrn.update(Bw, 1.0 / Bw, demo_stats_row=torch.zeros(2, FD, device="cuda"))


# ----------------------------------------------------------------------------- 8. learning check
def test_demonstration_term_reaches_the_optimiser(tmp_path):
    """clip_coeff = value_coeff = ent_coeff = 0, demo_coeff = 1: 30 mixed steps with clip + Adam (lr 1e-3) on one fixed
    demonstration minibatch beside random PPO rows; the demo NLL falls below half its starting value on both heads."""
    agent = make_agent(tmp_path)
    lrn = agent.learner
    lrn.cc, lrn.vc, lrn.ec = 0.0, 0.0, 0.0
    Bw = 16
    (ps, pt), (adv_s, adv_t) = ppo_storages(32, seed=10)
    demo, _host = random_demo(agent, 16, seed=16)
    idx = torch.arange(Bw)
    batches, entries = [(ps, idx, adv_s, pt, idx + 16, adv_t)], demo.batch(idx)
    rows = torch.zeros(30, 2, FD, device="cuda")
    for i in range(30):
        agent.update_policy_from_storages(batches, sync=False, demo=entries, demo_coeff=1.0, demo_value_coeff=0.0,
                                          demo_stats_row=rows[i])
        lrn.clip_adam(lr=1e-3, max_grad_norm=250.0)
    nll = rows[:, :, 1].cpu()
    for hd in range(2):
        print("head %d: demo NLL %.4f -> %.4f" % (hd, float(nll[0, hd]), float(nll[-1, hd])))
        assert float(nll[-1, hd]) < 0.5 * float(nll[0, hd])
    assert bool(torch.isfinite(agent.arena.params).all())


# ----------------------------------------------------------------------------- 9. train_vec
def test_train_vec_with_a_demo_mix_key(tmp_path):
    from cadre_amd import hip
    from ppo_agent import train as train_mod
    from tests.helpers import SyntheticEnv, topology_cfgs
    paths = record_episodes(tmp_path / "demos")

    def run(tag, **extra):
        lines = []

        class Logger(object):
            def log(self, s):
                lines.append(s)
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / tag), T=8, episodes=2)
        train_cfg.update(extra)
        os.makedirs(str(tmp_path / tag), exist_ok=True)
        agent = train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=SyntheticEnv, logger=Logger())
        torch.cuda.synchronize()
        return agent, lines
    plain, plain_lines = run("a", log_stats=True, demo_mix=None)
    mixed, lines = run("b", log_stats=True, demo_mix=dict(episodes=os.path.dirname(paths[0]), coeff=("linear", 1.0, 0.0)))
    assert sum("demo nll" in s for s in lines) == 2 and not any("demo nll" in s for s in plain_lines)
    lrn = mixed.learner
    assert lrn.device_hyper and float(lrn._hp[hip.HP_DEMO_COEFF]) == 0.5 and float(lrn._hp[hip.HP_DEMO_VALUE_COEFF]) == 0.0
    assert not plain.learner.device_hyper and lrn.loss_mode == "ppo"
    assert mixed.arena.step == plain.arena.step == 4
    assert bool(torch.isfinite(mixed.arena.params).all()) and not torch.equal(mixed.arena.params, plain.arena.params)
