"""Class-aware NMS with a detection cap, restated from the class-agnostic oracle (helper of test_nms_cls_cpu.py and
test_gpu_nms_cls.py; no test of its own).

Candidates are formed as oracle.post.decode forms them (max class score > conf, the first maximal class, xywh -> xyxy).
A candidate is kept iff no earlier kept candidate of its own label has !(IoU <= thr) with it, which is the
class-agnostic oracle NMS run on each label's candidates alone; the kept indices are merged by (score descending,
filtered index ascending) and cut to the first max_det (0: no cap)."""
import numpy as np

from oracle import post as op

# seed, B, N, nc, conf, iou: each the smallest input that reaches one branch of csrc/nms.hip
CASES = {
    11: (11, 1, 130, 5, 0.25, 0.45),      # bitmask path, one scan group
    12: (12, 2, 600, 5, 0.25, 0.45),      # bitmask path, far rows, > SCAN_RB kept rows in a group
    13: (13, 1, 8400, 5, 0.25, 0.45),     # bitmask path, all three far words per lane
    14: (14, 1, 8400, 80, 0.001, 0.7),    # rowmax_wave_kernel (C > 64), very dense keeps
    15: (15, 9, 17, 5, 0.25, 0.45),       # image kernel (B > 8), tiny K
    16: (16, 9, 127, 3, 0.0, 0.45),       # image kernel, N just under the bitmask floor
    19: (19, 9, 2000, 80, 0.001, 0.7),    # image kernel register form, long greedy loop
    17: (17, 1, 9601, 5, 0.0, 0.45),      # just past BM_MAX_WN, K > 8192: large-K form, LDS sort
    18: (18, 1, 16500, 5, 0.0, 0.45),     # K > SORT_LDS_KEYS: global-memory sort
}
# the cases the cap tests run, with their caps
MAX_DET = {13: (1, 300), 19: (1, 300)}

_PREDS = {}


def case_pred(seed):
    """The case's synth_eval_preds tensor (built once per process; treat as read-only)."""
    from datasets.synthetic import synth_eval_preds
    if seed not in _PREDS:
        s, B, N, nc, _, _ = CASES[seed]
        _PREDS[seed] = synth_eval_preds(B, N, nc=nc, seed=s)
    return _PREDS[seed]


_REFS = {}


def case_ref(seed):
    """decode_cls of the case, uncapped (computed once per process; a cap is a prefix of it)."""
    if seed not in _REFS:
        _, _, _, _, conf, iou = CASES[seed]
        _REFS[seed] = decode_cls(case_pred(seed).numpy(), 640, conf, iou)
    return _REFS[seed]


def candidates(p, conf):
    """One image (N, 4+C) -> xyxy, score, label of the rows whose max class score > conf, in row order."""
    p = np.asarray(p, np.float32)
    cls = p[:, 4:]
    mx = cls.max(1)
    lab = cls.argmax(1)
    m = mx > np.float32(conf)
    xywh, mx, lab = p[m, :4], mx[m], lab[m]
    half_w = xywh[:, 2] / np.float32(2)
    half_h = xywh[:, 3] / np.float32(2)
    xyxy = np.stack([xywh[:, 0] - half_w, xywh[:, 1] - half_h, xywh[:, 0] + half_w, xywh[:, 1] + half_h], 1)
    return xyxy.astype(np.float32).reshape(-1, 4), mx, lab.astype(np.int64)


def merge(keeps, scores):
    """Kept filtered indices of several NMS runs -> one list ordered by (score descending, index ascending)."""
    keep = np.concatenate([np.asarray(k, np.int64) for k in keeps]) if keeps else np.zeros(0, np.int64)
    return keep[np.lexsort((keep, -scores[keep].astype(np.float64)))]


def nms_cls(boxes, scores, labels, thr, max_det=0):
    """Per-label oracle NMS, merged; indices into boxes."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32)
    labels = np.asarray(labels)
    keeps = []
    for lb in np.unique(labels):
        idx = np.nonzero(labels == lb)[0]
        keeps.append(idx[op.nms(boxes[idx], scores[idx], thr)])
    keep = merge(keeps, scores)
    return keep[:max_det] if max_det > 0 else keep


def decode_cls(pred, img_size, conf, iou_thr, max_det=0):
    """pred (B, N, 4+C) -> per image (boxes, scores, labels, filtered indices), class-aware."""
    outs = []
    for p in np.asarray(pred, np.float32):
        xyxy, mx, lab = candidates(p, conf)
        keep = nms_cls(xyxy, mx, lab, iou_thr, max_det)
        bx = np.clip(xyxy[keep] / np.float32(img_size), 0.0, 1.0).astype(np.float32).reshape(-1, 4)
        outs.append((bx, mx[keep], lab[keep], keep))
    return outs
