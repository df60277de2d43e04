"""The numpy restatement of the top-k task-aligned assigner (tests/tal_topk_ref.py) held to hand-worked
answers and to the rule's properties, so the GPU tests can hold the kernels to the restatement."""
import numpy as np
import pytest

import tal_topk_cases as tc
import tal_topk_ref as tr


def _run(case, k, alpha=1.0, beta=1.0, eps=1e-9):
    return tr.assign(case["scores"], case["boxes"], case["anc"], case["labels"], case["gboxes"], case["mask"], k,
                     alpha, beta, eps)


@pytest.fixture(scope="module")
def case():
    return tc.explicit_case()


def test_iou_restates_the_oracle_iou():
    """iou_f32 is oracle.loss.bbox_iou (the kernel's iou_xyxy op order) clamped at 0, bit for bit."""
    import torch
    from oracle import loss as ol
    c = tc.random_case(3)
    for b in range(2):
        for g in range(c["gboxes"].shape[1]):
            want = ol.bbox_iou(torch.from_numpy(c["boxes"][b]), torch.from_numpy(c["gboxes"][b, g])[None]).clamp(0)
            np.testing.assert_array_equal(tr.iou_f32(c["boxes"][b], c["gboxes"][b, g]), want.squeeze(-1).numpy())


@pytest.mark.parametrize("k", [1, 2, 3, 10, 441])
def test_hand_worked_scenes(case, k):
    """More than k in-box anchors (G0: the k best, the a2 / a3 metric tie to the lower anchor), fewer than k (G1: both,
    the zero-metric one included), none (G2: no positive, nothing forced), an invalid slot holding G0's box, one anchor
    claimed by two gts with different IoUs (a7 -> G3) and with equal IoUs (image 1's a9 -> the lower slot), k = 1 (G4
    loses its only candidate and ends empty) and k >= A."""
    res = _run(case, k)
    for b in range(2):
        want = tc.HAND[k][b]
        for a in range(tc.NH):
            if a in want:
                assert res[b]["fg"][a] and res[b]["tgi"][a] == want[a][0], (k, b, a)
                assert res[b]["norm"][a] == np.float32(want[a][1]), (k, b, a, res[b]["norm"][a])
            else:
                assert not res[b]["fg"][a] and res[b]["tgi"][a] == 0 and res[b]["norm"][a] == 0, (k, b, a)
    r0 = res[0]
    assert not r0["cand"][2] and not r0["inbox"][2].any()                 # G2: valid, no in-box anchor, no positives
    assert not (r0["fg"] & (r0["tgi"] == 2)).any()
    assert not r0["cand"][5] and not (r0["fg"] & (r0["tgi"] == 5)).any()    # the invalid slot takes nothing
    assert r0["cand"][0] == [1, 2, 3, 0, 4][:k]                           # rank order, the tie to the lower anchor
    assert r0["cand"][1] == [5, 6][:k]
    assert not r0["fg"][tc.NH:].any()                                     # image 0's grid anchors lie in no gt
    if k == 441:                                                      # k >= A: every in-box anchor of every valid gt
        for r in res:
            for g in range(tc.M):
                assert sorted(r["cand"][g]) == list(np.nonzero(r["inbox"][g])[0])


def test_case_exercises_ties_and_both_sides_of_k(case):
    res = _run(case, 10)[1]
    for i, j in case["dup"]:                   # the duplicated rows tie inside image 1's large box
        assert res["inbox"][2, i] and res["inbox"][2, j] and res["metric"][2, i] == res["metric"][2, j]
    n_in = res["inbox"].sum(1)
    assert n_in[2] > 10 and n_in[3] > 10 and 0 < n_in[4] < 10
    claims = np.zeros(tc.A, int)
    for g in range(tc.M):
        claims[res["cand"][g]] += 1
    assert (claims[tc.NH:] > 1).any()          # grid anchors claimed by both overlapping boxes


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("k,alpha,beta", [(1, 1.0, 1.0), (4, 0.5, 4.0), (13, 1.0, 6.0)])
def test_properties_on_random_inputs(seed, k, alpha, beta):
    c = tc.random_case(seed)
    flat = 0
    for b, r in enumerate(_run(c, k, alpha, beta)):
        assert r["fg"][r["tgi"] != 0].all()                                         # background rows carry tgi 0
        assert (r["norm"][~r["fg"]] == 0).all()
        for g in range(c["gboxes"].shape[1]):
            mine = np.nonzero(r["fg"] & (r["tgi"] == g))[0]
            n_in = int(r["inbox"][g].sum())
            assert len(r["cand"][g]) == (min(k, n_in) if c["mask"][b, g] else 0)
            assert len(mine) <= k                                                   # at most k anchors per gt
            assert r["inbox"][g, mine].all() and set(mine) <= set(r["cand"][g])     # positives are in-box candidates
            if not c["mask"][b, g]:
                assert len(mine) == 0
            elif len(mine) and r["metric"][g, mine].max() > 0:
                # the best-aligned anchor of a gt carries the gt's best IoU as its target score: max norm =
                # maxo * maxm / (maxm + eps).  The formula's own eps = 1e-9 takes maxo * eps / (maxm + eps) off it:
                # below 1e-6 once maxm >= 1e-3, where max norm == maxo within 1e-6 as the rule promises; a smaller
                # metric (iou^4 or iou^6 of a poor box) is held to the formula's value instead (1.05e-5 off maxo
                # at maxm = 6e-6, for one)
                maxm, maxo = float(r["metric"][g, mine].max()), float(r["iou"][g, mine].max())
                got = float(r["norm"][mine].max())
                assert abs(got - maxo * maxm / (maxm + 1e-9)) <= 1e-6
                if maxm >= 1e-3:
                    flat += 1
                    assert abs(got - maxo) <= 1e-6
        # at most one gt per anchor: fg / tgi are single-valued by construction; every claimed anchor is foreground
        claimed = sorted({a for cg in r["cand"] for a in cg})
        assert claimed == list(np.nonzero(r["fg"])[0])
        for a in claimed:                       # the winner has the largest IoU among the claimants, lowest g on ties
            cl = [g for g in range(len(r["cand"])) if a in r["cand"][g]]
            best = max(cl, key=lambda g: (float(r["iou"][g, a]), -g))
            assert r["tgi"][a] == best
    assert flat > 0


def test_trainer_flags_and_constructor_argument():
    """--assigner / --tal-topk parse (defaults: inbox, 10; an unknown assigner is refused), and v8DetectionLoss takes
    `assigner` ("inbox" | "topk", anything else a ValueError) without tal_topk alone switching the mode."""
    import torch.nn as nn
    import train_yolo11_cuda as T
    from models import Detect
    from losses import v8DetectionLoss
    ns = T.build_parser().parse_args([])
    assert (ns.assigner, ns.tal_topk) == ("inbox", 10)
    ns = T.build_parser().parse_args(["--assigner", "topk", "--tal-topk", "13"])
    assert (ns.assigner, ns.tal_topk) == ("topk", 13)
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--assigner", "atss"])

    class Stub(nn.Module):
        def __init__(self):
            super().__init__()
            self.det = Detect(3, (64, 128, 256))
            self.det.stride = [8.0, 16.0, 32.0]
    stub = Stub()
    assert v8DetectionLoss(stub, tal_topk=10).assign_mode == "inbox"
    crit = v8DetectionLoss(stub, tal_topk=7, assigner="topk")
    assert crit.assign_mode == "topk" and crit.assigner.use_topk and crit.assigner.topk == 7
    with pytest.raises(ValueError, match="assigner"):
        v8DetectionLoss(stub, assigner="atss")
