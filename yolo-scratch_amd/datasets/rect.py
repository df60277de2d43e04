"""Sampler of rectangular validation: images in the order of their aspect ratio.

A batch's frame is the minimal stride-multiple rectangle that holds all of its images
(datasets.letterbox.rect_frame), so a batch of one portrait and one landscape image needs the full square.
Walking the set by h0 / w0 puts images of like shape next to each other: batches of neighbours share a small
frame, and the whole set touches each frame in one run.
"""
from __future__ import annotations

import torch


class RectSampler(torch.utils.data.Sampler):
    """The inner sampler's indices, ordered by `ratios[index]` (h0 / w0) ascending; ties keep the inner order.

    `inner`: any iterable of indices, such as range(n) for the ordered val set or a ValShard under data
    parallelism: each rank sorts its own shard, so no image is yielded by two ranks.  `ratios`: one number per
    dataset index.  The indices are materialised at every __iter__."""

    def __init__(self, inner, ratios):
        self.inner, self.ratios = inner, [float(r) for r in ratios]

    def __iter__(self):
        idx = list(self.inner)
        return iter(sorted(idx, key=lambda i: self.ratios[i]))       # sorted() is stable

    def __len__(self):
        return len(self.inner)
