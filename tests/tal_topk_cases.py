"""Inputs of the top-k assigner tests (CPU restatement and GPU kernels): one explicit-tensor case that carries the
hand-worked scenes, and random cases for the property checks.

explicit_case(): B = 2, A = 441 (10 hand-placed anchors, then a 21x16 grid at stride 8, 10x8 at stride 16 and 5x3 at
stride 32 — not a multiple of 64 or 256), M = 6 with one invalid slot per image, nc = 3.  The hand scenes live at
x >= 1000, away from the grid (x < 168): with alpha = beta = 1 their IoUs, scores and metrics are powers of two, so
every answer in HAND is exact in fp32 (the 1e-7 / 1e-9 epsilons round away at these magnitudes).

Hand anchors (image 0 unless noted; s = score at the gt's label):
  a0..a4 centres inside G0 = [1000,0,1010,10] (label 0), IoU .25, 1, .5, .5, .125, s = 1; a3's row duplicates a2's
  a5, a6 inside G1 = [1100,0,1110,10] (label 1): a5 IoU .5, s .5 (metric .25); a6's box is disjoint (metric 0)
  G2 = [1200,0,1201,1] holds no anchor centre
  a7 inside G3 = [1300,0,1310,10] and G4 = [1300,0,1310,20] (labels 0): IoU 1 and .5, s 1
  a8 inside G4 only: IoU .25, s .5 (metric .125)
  slot 5: G0's box again with mask 0
  image 1: a9 inside G0' = G1' = [1400,0,1410,10] (labels 0, 1): IoU .5 with both, s 1 and .5; slots 2-4 are three
  boxes over the grid (large, overlapping the large one, small), slot 5 zero padding with mask 0."""
import numpy as np

F = np.float32
NH = 10
A = 441
NC = 3
M = 6

# HAND[k] = {image: {anchor: (tgi, norm)}} for the hand anchors that are foreground; every other hand anchor is
# background.  k = 441 stands for any k >= A.
_G0_ALL = {0: (0, .25), 1: (0, 1.0), 2: (0, .5), 3: (0, .5), 4: (0, .125)}
HAND = {
    1: {0: {1: (0, 1.0), 5: (1, .5), 7: (3, 1.0)},               # G4's only candidate a7 goes to G3: G4 ends empty
        1: {9: (0, .5)}},
    2: {0: {1: (0, 1.0), 2: (0, .5), 5: (1, .5), 6: (1, 0.0), 7: (3, 1.0), 8: (4, .25)},
        1: {9: (0, .5)}},
    3: {0: {1: (0, 1.0), 2: (0, .5), 3: (0, .5), 5: (1, .5), 6: (1, 0.0), 7: (3, 1.0), 8: (4, .25)},
        1: {9: (0, .5)}},
    10: {0: {**_G0_ALL, 5: (1, .5), 6: (1, 0.0), 7: (3, 1.0), 8: (4, .25)},
         1: {9: (0, .5)}},
}
HAND[441] = HAND[10]


def grid_anchors():
    pts = []
    for (h, w, s) in ((16, 21, 8.0), (8, 10, 16.0), (3, 5, 32.0)):
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pts.append(np.stack(((xs.ravel() + 0.5) * s, (ys.ravel() + 0.5) * s), 1))
    return np.concatenate(pts).astype(F)


def explicit_case():
    rng = np.random.default_rng(7)
    anc = np.zeros((A, 2), F)
    anc[NH:] = grid_anchors()
    assert len(anc) == A == NH + 336 + 80 + 15
    boxes = np.zeros((2, A, 4), F)
    scores = np.zeros((2, A, NC), F)
    # random predictions on the grid, both images: a box around the anchor, scores U(0, 1)
    c = anc[NH:]
    for b in range(2):
        e = rng.uniform(2.0, 40.0, (A - NH, 4)).astype(F)
        boxes[b, NH:] = np.concatenate((c - e[:, :2], c + e[:, 2:]), 1)
        scores[b, NH:] = rng.uniform(0.0, 1.0, (A - NH, NC)).astype(F)
    # duplicated prediction rows (equal IoU and score: equal metrics, decided by the anchor index): neighbours
    # inside image 1's large box; the boxes are copied, so the duplicates are the same box, not a shifted one
    dup = [(NH + 21 * 4 + 5, NH + 21 * 4 + 6), (NH + 21 * 6 + 8, NH + 21 * 7 + 8),
           (NH + 336 + 10 * 2 + 3, NH + 336 + 10 * 2 + 4)]
    for i, j in dup:
        boxes[1, j] = boxes[1, i]
        scores[1, j] = scores[1, i]
    hand_c = [(1001, 1), (1002, 2), (1003, 3), (1004, 4), (1005, 5), (1101, 1), (1102, 2), (1305, 5), (1305, 15),
              (1405, 5)]
    anc[:NH] = np.array(hand_c, F)
    hb = [[1000, 0, 1010, 2.5], [1000, 0, 1010, 10], [1000, 0, 1010, 5], [1000, 0, 1010, 5], [1000, 0, 1010, 1.25],
          [1100, 0, 1110, 5], [1100, 20, 1110, 30], [1300, 0, 1310, 10], [1300, 0, 1310, 5], [1400, 0, 1410, 5]]
    hs = [[1, 0, 0]] * 5 + [[0, .5, 0], [0, .5, 0], [1, 0, 0], [.5, 0, 0], [1, .5, 0]]
    boxes[:, :NH] = np.array(hb, F)
    scores[:, :NH] = np.array(hs, F)
    gboxes = np.zeros((2, M, 4), F)
    labels = np.zeros((2, M), F)
    mask = np.ones((2, M), F)
    gboxes[0] = [[1000, 0, 1010, 10], [1100, 0, 1110, 10], [1200, 0, 1201, 1], [1300, 0, 1310, 10],
                 [1300, 0, 1310, 20], [1000, 0, 1010, 10]]
    labels[0] = [0, 1, 2, 0, 0, 0]
    gboxes[1] = [[1400, 0, 1410, 10], [1400, 0, 1410, 10], [20, 16, 120, 100], [36, 24, 136, 112], [8, 8, 20, 20],
                 [0, 0, 0, 0]]
    labels[1] = [0, 1, 2, 2, 0, 0]
    mask[:, 5] = 0
    return dict(scores=scores, boxes=boxes, anc=anc, labels=labels, gboxes=gboxes, mask=mask, dup=dup)


def random_case(seed, B=2, m=5, nc=4, imgsz=96):
    """Random explicit tensors on the three-level grid of an imgsz image; a padded (invalid) slot per image."""
    rng = np.random.default_rng(seed)
    pts = []
    for s in (8, 16, 32):
        n = imgsz // s
        ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        pts.append(np.stack(((xs.ravel() + 0.5) * s, (ys.ravel() + 0.5) * s), 1))
    anc = np.concatenate(pts).astype(F)
    a = len(anc)
    e = rng.uniform(1.0, imgsz / 3, (B, a, 4)).astype(F)
    boxes = np.concatenate((anc[None] - e[..., :2], anc[None] + e[..., 2:]), 2)
    scores = rng.uniform(0.0, 1.0, (B, a, nc)).astype(F)
    ctr = rng.uniform(0.1, 0.9, (B, m, 2)) * imgsz
    wh = np.exp(rng.uniform(np.log(0.04), np.log(0.7), (B, m, 2))) * imgsz
    gboxes = np.clip(np.concatenate((ctr - wh / 2, ctr + wh / 2), 2), 0, imgsz).astype(F)
    labels = rng.integers(0, nc, (B, m)).astype(F)
    mask = np.ones((B, m), F)
    mask[:, -1] = 0
    return dict(scores=scores, boxes=boxes, anc=anc, labels=labels, gboxes=gboxes, mask=mask)
