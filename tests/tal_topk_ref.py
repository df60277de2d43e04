"""Numpy restatement of the top-k task-aligned assigner — TEST REFERENCE ONLY.

Steps 1-4 as the kernels' contract states them, per image:
  1. per valid gt g and anchor a: inbox = min(l, t, r, b) > 1e-9; iou = the project's plain xyxy IoU clamped at 0,
     in fp32 and the kernel's op order; metric = s^alpha * iou^beta in fp32 (an exponent of exactly 1 is the value,
     0.5 the square root, anything else pow), s the score at g's label;
  2. g's candidates: its k in-box anchors of largest metric, ties to the lowest anchor; fewer than k: all of them;
  3. an anchor's gt: the claiming gt of largest iou, ties to the lowest g; no claimant: background (tgi 0, norm 0);
  4. norm(a) = metric(a, g) * maxo(g) / (maxm(g) + eps), maxima over the anchors finally assigned to g.
Every decision uses the fp32 quantities; an fp64 metric (from the fp32 score and IoU) is returned beside them so a
test can measure how far apart the ranked metrics lie (`min_gaps`)."""
import numpy as np

F = np.float32
EPS_IOU = F(1e-7)
EPS_IN = F(1e-9)


def iou_f32(pb, gb):
    """IoU of boxes pb (A, 4) with one box gb (4,), fp32, iou_xyxy's op order (eps placement included), clamped at 0."""
    pb, gb = pb.astype(F), gb.astype(F)
    w1, h1 = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1] + EPS_IOU
    w2, h2 = gb[2] - gb[0], gb[3] - gb[1] + EPS_IOU
    iw = np.minimum(pb[:, 2], gb[2]) - np.maximum(pb[:, 0], gb[0])
    ih = np.minimum(pb[:, 3], gb[3]) - np.maximum(pb[:, 1], gb[1])
    iw = np.where(iw < 0, F(0), iw)
    ih = np.where(ih < 0, F(0), ih)
    inter = iw * ih
    uni = w1 * h1 + w2 * h2 - inter + EPS_IOU
    iou = inter / uni
    return np.where(iou < 0, F(0), iou).astype(F)


def _pow(v, e, dtype):
    if e == 1.0:
        return v.astype(dtype)
    if e == 0.5:
        return np.sqrt(v.astype(dtype))
    return np.power(v.astype(dtype), dtype(e))


def assign_image(scores, boxes, anc, labels, gboxes, valid, k, alpha, beta, eps):
    """One image.  scores (A, nc) probabilities, boxes (A, 4) and anc (A, 2) pixels, labels (M,), gboxes (M, 4),
    valid (M,) truthy flags.  -> dict: fg (A,) bool, tgi (A,) int64, norm (A,) fp32, cand (list of M anchor lists, in
    rank order), inbox (M, A) bool, iou / metric (M, A) fp32, metric64 (M, A) fp64."""
    scores, boxes, anc, gboxes = (np.asarray(x, dtype=F) for x in (scores, boxes, anc, gboxes))
    A, nc = scores.shape
    M = gboxes.shape[0]
    inbox = np.zeros((M, A), bool)
    iou = np.zeros((M, A), F)
    metric = np.zeros((M, A), F)
    metric64 = np.zeros((M, A), np.float64)
    cand = [[] for _ in range(M)]
    for g in range(M):
        if not valid[g]:
            continue
        gb = gboxes[g]
        sides = np.stack((anc[:, 0] - gb[0], anc[:, 1] - gb[1], gb[2] - anc[:, 0], gb[3] - anc[:, 1]), 1)
        inbox[g] = sides.min(1) > EPS_IN
        iou[g] = iou_f32(boxes, gb)
        s = scores[:, min(max(int(labels[g]), 0), nc - 1)]
        metric[g] = _pow(s, alpha, F) * _pow(iou[g], beta, F)
        metric64[g] = _pow(s, alpha, np.float64) * _pow(iou[g], beta, np.float64)
        ins = [int(a) for a in np.nonzero(inbox[g])[0]]
        cand[g] = sorted(ins, key=lambda a: (-float(metric[g, a]), a))[:k]
    fg = np.zeros(A, bool)
    tgi = np.zeros(A, np.int64)
    best = np.full(A, -1.0)
    for g in range(M):                      # ascending g, strict >: equal IoUs keep the lowest g
        for a in cand[g]:
            if float(iou[g, a]) > best[a]:
                best[a] = float(iou[g, a])
                tgi[a] = g
                fg[a] = True
    norm = np.zeros(A, F)
    for g in range(M):
        mine = np.nonzero(fg & (tgi == g))[0]
        if len(mine) == 0:
            continue
        maxm, maxo = metric[g, mine].max(), iou[g, mine].max()
        norm[mine] = metric[g, mine] * maxo / (maxm + F(eps))
    return dict(fg=fg, tgi=tgi, norm=norm, cand=cand, inbox=inbox, iou=iou, metric=metric, metric64=metric64)


def assign(scores, boxes, anc, labels, gboxes, valid, k, alpha, beta, eps):
    """A batch: scores (B, A, nc), boxes (B, A, 4), anc (A, 2), labels / valid (B, M), gboxes (B, M, 4) -> a list of
    assign_image results."""
    return [assign_image(scores[b], boxes[b], anc, labels[b], gboxes[b], valid[b], k, alpha, beta, eps)
            for b in range(len(scores))]


def min_gaps(res, k):
    """Smallest relative gaps that a ranking of one image rests on, from the fp64 metric and the fp32 IoU:
    (between every gt's k-th and (k+1)-th in-box metric, between every anchor's two best claiming IoUs).  A pair
    of equal values has gap 0 (two zeros included); inf where no such pair exists."""
    rank_gap = claim_gap = np.inf
    M = len(res["cand"])
    for g in range(M):
        ins = np.nonzero(res["inbox"][g])[0]
        if len(ins) > k:
            m = np.sort(res["metric64"][g, ins])[::-1]
            rank_gap = min(rank_gap, (m[k - 1] - m[k]) / m[k - 1] if m[k - 1] > 0 else 0.0)
    claims = {}
    for g in range(M):
        for a in res["cand"][g]:
            claims.setdefault(a, []).append(float(res["iou"][g, a]))
    for v in claims.values():
        if len(v) > 1:
            v = sorted(v, reverse=True)
            claim_gap = min(claim_gap, (v[0] - v[1]) / v[0] if v[0] > 0 else 0.0)
    return rank_gap, claim_gap


def oracle_assign(k, alpha=0.5, beta=4.0, eps=1e-9, record=None):
    """A drop-in for oracle.loss.assign (same arguments and 5-tuple) that assigns by this restatement; every image's
    assign_image result is appended to `record`."""
    import torch

    @torch.no_grad()
    def fn(pd_scores, pd_bboxes, anc, gt_labels, gt_bboxes, mask_gt):
        B, A, nc = pd_scores.shape
        M = gt_bboxes.shape[1]
        if M == 0:
            return (torch.full((B, A), nc, dtype=torch.long), torch.zeros(B, A, 4), torch.zeros(B, A, nc),
                    torch.zeros(B, A), torch.zeros(B, A))
        res = assign(pd_scores.numpy(), pd_bboxes.numpy(), anc.numpy(), gt_labels.numpy(), gt_bboxes.numpy(),
                     mask_gt.numpy(), k, alpha, beta, eps)
        if record is not None:
            record.extend(res)
        fg = torch.from_numpy(np.stack([r["fg"] for r in res]))
        tgi = torch.from_numpy(np.stack([r["tgi"] for r in res]))
        norm = torch.from_numpy(np.stack([r["norm"] for r in res]))
        flat = tgi + torch.arange(B)[:, None] * M
        t_labels = gt_labels.flatten()[flat].clamp(0, nc)
        t_bboxes = gt_bboxes.reshape(-1, 4)[flat]
        ts = torch.zeros(B, A, nc).scatter_(2, t_labels.unsqueeze(-1).long(), 1)
        ts = torch.where(fg[:, :, None], ts, torch.zeros(()))
        return t_labels, t_bboxes, ts * norm[..., None], fg, tgi
    return fn
