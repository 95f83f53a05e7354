"""CPU: ordinal policy heads — the rank helper and the config rules, the five `_ord` entry points (declared, bound, bad
arguments rejected before any launch) and the float64 statement of the math (tests/ordinal_ref.py) itself."""
import pytest
import torch

from tests import ordinal_ref


def shipped_steer():
    """The shipped table's shape: bins 0..16 = -8/16 .. 8/16 ascending, then +9/16, -9/16, ... +15/16, -15/16, +1, -1."""
    ctl = {i: (i - 8) / 16.0 for i in range(17)}
    for n, v in enumerate(range(9, 17)):
        ctl[17 + 2 * n] = v / 16.0
        ctl[18 + 2 * n] = -v / 16.0
    return ctl


THROTTLE = {0: [0, 0], 1: [0, 1], 2: [0.6, 0]}


def test_ordinal_rank_of_the_shipped_tables():
    from ppo_agent.agent import ordinal_rank
    ctl = shipped_steer()
    assert len(ctl) == 33 and ctl[17] == 9 / 16 and ctl[18] == -9 / 16 and ctl[31] == 1.0 and ctl[32] == -1.0
    rank = ordinal_rank(ctl)
    assert sorted(rank) == list(range(33))
    assert (rank[0], rank[16], rank[17], rank[18], rank[31], rank[32]) == (8, 24, 25, 7, 32, 0)
    by_rank = sorted(range(33), key=lambda k: rank[k])
    vals = [ctl[k] for k in by_rank]
    assert vals == sorted(vals)
    assert ordinal_rank({i: (i - 16) / 16.0 for i in range(33)}) == list(range(33))
    assert ordinal_rank(THROTTLE) == [1, 0, 2]
    assert ordinal_rank({0: 3.0, 1: 1.0, 2: 2.0}, key=lambda v: -v) == [0, 2, 1]


def test_ordinal_rank_and_config_rejections():
    from cadre_amd.hip import CadreHipError
    from ppo_agent.agent import ordinal_rank, resolve_ordinal
    with pytest.raises(CadreHipError):
        ordinal_rank({0: 0.5, 1: 0.25, 2: 0.5})                      # duplicate keys: no strict order
    with pytest.raises(CadreHipError):
        ordinal_rank({0: [0.5, 0.5], 1: [0, 0], 2: [0.6, 0]})        # throttle - brake ties
    n_out = {"steer": 5, "throttle": 3}
    for bad in ([0, 1, 2, 3, 3], [0, 1, 2, 3], [1, 2, 3, 4, 5], [0, 1, 2, 3, 4.5], "abcde", [-1, 0, 1, 2, 3]):
        with pytest.raises(CadreHipError):
            resolve_ordinal({"steer": bad}, n_out)
    with pytest.raises(CadreHipError):
        resolve_ordinal({"wheel": True}, n_out)
    with pytest.raises(CadreHipError):
        resolve_ordinal(True, n_out, {"steer": {0: 0.0, 1: 1.0}, "throttle": THROTTLE})       # table size != head size
    # off / on / per head
    assert resolve_ordinal(None, n_out) is None and resolve_ordinal(False, n_out) is None
    assert resolve_ordinal({"steer": False, "throttle": False}, n_out) is None
    assert resolve_ordinal(True, n_out) == [[0, 1, 2, 3, 4], [0, 1, 2]]                        # no tables: identity
    ctl = {"steer": {0: 0.0, 1: 0.5, 2: -0.5, 3: 1.0, 4: -1.0}, "throttle": THROTTLE}
    assert resolve_ordinal(True, n_out, ctl) == [[2, 3, 1, 4, 0], [1, 0, 2]]
    assert resolve_ordinal({"steer": True}, n_out, ctl) == [[2, 3, 1, 4, 0], None]
    assert resolve_ordinal({"steer": [4, 3, 2, 1, 0], "throttle": True}, n_out, ctl) == [[4, 3, 2, 1, 0], [1, 0, 2]]


def test_ord_entry_points_reject_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15            # entry points are only added
    for name in ("cadre_ppo_loss_ord", "cadre_sample_ord", "cadre_sample_rows_ord", "cadre_categorical_eval_ord",
                 "cadre_categorical_dist_ord"):
        assert name in hip.SYMBOLS and hasattr(L, name)
    P = 16                                                           # (never dereferenced: rejected before any launch)
    loss = [P, 64, 64 * 64, P, 64, 64 * 64, P, P, P, P, P, P, 64, 4, 33, 3, None, 0.1, 0.1, 1.0, 0.01, 1 / 64, P, P, P, P, None,
            None, 0, None, 0.0, None, P]
    ORD = len(loss) - 1

    def bad_loss(i, v, text=b"cadre_ppo_loss_ord"):
        a = list(loss)
        a[i] = v
        assert L.cadre_ppo_loss_ord(*a, None) == -1 and text in L.cadre_last_error(), (i, v, L.cadre_last_error())
    bad_loss(ORD, None, b"rank table")
    bad_loss(14, 65); bad_loss(15, 65); bad_loss(1, 32); bad_loss(1, 65); bad_loss(13, 0); bad_loss(0, None)
    bad_loss(16, 20, b"hyper-parameter block")                       # misaligned block
    for i, v in ((28, 7), (29, None)):                               # a stats row with F < 8 / without partials scratch
        a = list(loss)
        a[27], a[28], a[29] = P, 16, P
        a[i] = v
        assert L.cadre_ppo_loss_ord(*a, None) == -1 and b"stats" in L.cadre_last_error()
    a = list(loss)
    a[27], a[28], a[29], a[30] = P, 16, P, 0.01                      # gate armed without a flag
    assert L.cadre_ppo_loss_ord(*a, None) == -1

    def check(fn, name, good, ord_i, k_i, ld_i):
        for i, v, text in ((ord_i, None, b"rank table"), (k_i, 65, name), (k_i, 0, name), (ld_i, 32, name), (0, None, name)):
            a = list(good)
            a[i] = v
            assert fn(*a, None) == -1 and text in L.cadre_last_error() and name in L.cadre_last_error(), (name, i, v)
    check(L.cadre_sample_ord, b"cadre_sample_ord", [P, 64, P, 64, 4, 33, P, P, P], 8, 5, 1)
    check(L.cadre_categorical_eval_ord, b"cadre_categorical_eval_ord", [P, 64, P, 4, 33, P, P, P], 7, 4, 1)
    check(L.cadre_categorical_dist_ord, b"cadre_categorical_dist_ord", [P, 64, 4, 33, P, P, P, P], 7, 3, 1)
    check(L.cadre_sample_rows_ord, b"cadre_sample_rows_ord", [P, 64, 5 * 64, P, P, 5, 4, P, 33, 3, P, P, P, P], 13, 8, 1)
    rows = [P, 64, 5 * 64, P, P, 5, 4, P, 33, 3, P, P, P, P]
    for i, v in ((9, 65), (6, 17), (2, 64)):
        a = list(rows)
        a[i] = v
        assert L.cadre_sample_rows_ord(*a, None) == -1


def test_ordinal_ref_uniform_at_zero_and_monotone_meaning():
    for K, rank in ((5, [2, 3, 1, 4, 0]), (1, [0]), (33, list(range(33)))):
        lgn = ordinal_ref.normalised_logits(torch.zeros(3, K, dtype=torch.float64), rank)
        assert torch.allclose(lgn.exp(), torch.full((3, K), 1.0 / K, dtype=torch.float64), atol=1e-12)
    # all threshold units far on: the mass sits on the TOP rank, i.e. on the bin whose rank is K - 1
    rank = [2, 3, 1, 4, 0]
    p = ordinal_ref.normalised_logits(torch.full((1, 5), 6.0, dtype=torch.float64), rank).exp()[0]
    assert int(p.argmax()) == rank.index(4)
    p = ordinal_ref.normalised_logits(torch.full((1, 5), -6.0, dtype=torch.float64), rank).exp()[0]
    assert int(p.argmax()) == rank.index(0)


def test_ordinal_ref_gradient_matches_finite_difference_and_closed_form():
    g = torch.Generator().manual_seed(0)
    K, rank = 5, [2, 3, 1, 4, 0]
    x = (torch.randn(K, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    coef = torch.randn(K, generator=g, dtype=torch.float64)

    def f(v):
        lgn = ordinal_ref.normalised_logits(v.view(1, K), rank)[0]
        return (coef * lgn).sum() + 0.3 * ordinal_ref.entropy(lgn.view(1, K))[0]
    f(x).backward()
    h = 1e-6
    fd = torch.zeros(K, dtype=torch.float64)
    for j in range(K):
        e = torch.zeros(K, dtype=torch.float64)
        e[j] = h
        fd[j] = (f(x.detach() + e) - f(x.detach() - e)) / (2 * h)
    assert float((x.grad - fd).abs().max()) < 1e-8 * max(1.0, float(fd.abs().max()))
    # the closed form the kernels implement: alpha_j sum_{r >= j} G_r - beta_j sum_{r < j} G_r, G_r = g_{bin[r]}
    z = ordinal_ref.ordinal_logits(x.detach().view(1, K), rank)[0].requires_grad_(True)
    lgn = z - z.logsumexp(0)
    ((coef * lgn).sum() + 0.3 * ordinal_ref.entropy(lgn.view(1, K))[0]).backward()
    gk = z.grad                                                      # d / d logit of bin k
    binv = [rank.index(r) for r in range(K)]
    G = gk[binv]
    s, t = torch.sigmoid(x.detach()), torch.sigmoid(-x.detach())
    alpha, beta = s * t / (s + ordinal_ref.EPS), s * t / (t + ordinal_ref.EPS)
    want = torch.stack([alpha[j] * G[j:].sum() - beta[j] * G[:j].sum() for j in range(K)])
    assert float((x.grad - want).abs().max()) < 1e-12


def test_module_torch_tail_equals_the_reference_statement():
    """The differentiable tail of Model.evaluate_actions (cumsum form) against the mask-matrix statement, float64."""
    from ppo_agent.models import ordinal_logits
    g = torch.Generator().manual_seed(1)
    for K in (1, 2, 3, 33, 64):
        rank = torch.randperm(K, generator=g).tolist()
        x = torch.randn(7, K, generator=g, dtype=torch.float64) * 4
        assert float((ordinal_logits(x, rank) - ordinal_ref.ordinal_logits(x, rank)).abs().max()) < 1e-11
