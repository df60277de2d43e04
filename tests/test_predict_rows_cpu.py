"""predict.py's label rows (`cls cx cy w h conf`) have no negative size, whatever order the corners come in: a head
whose randomly initialised, frozen DFL weight has a negative mean decodes boxes with x2 < x1 and y2 < y1."""
import torch


def test_rows_of_reversed_corners_are_the_extent():
    import predict as P
    ordinary = {"boxes": torch.tensor([[10.0, 20.0, 30.0, 60.0]]), "scores": torch.tensor([0.5]),
                "labels": torch.tensor([2])}
    assert P.txt_rows(ordinary, 80, 40) == ["2 0.500000 0.500000 0.500000 0.500000 0.500000"]
    for box in ([30.0, 60.0, 10.0, 20.0], [30.0, 20.0, 10.0, 60.0], [10.0, 60.0, 30.0, 20.0]):
        det = {**ordinary, "boxes": torch.tensor([box])}
        assert P.txt_rows(det, 80, 40) == P.txt_rows(ordinary, 80, 40), box
    # the box the rectangular-inference test met: corners 1.8 pixels apart, in reverse
    det = {"boxes": torch.tensor([[3.417, 38.408, 1.640, 36.623]]), "scores": torch.tensor([1e-6]),
           "labels": torch.tensor([1])}
    vals = [float(v) for v in P.txt_rows(det, 60, 100)[0].split()[1:]]
    assert all(0.0 <= v <= 1.0 for v in vals) and vals[2] > 0.0 and vals[3] > 0.0
