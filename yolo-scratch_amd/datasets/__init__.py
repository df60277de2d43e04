"""Data path: the reference's crater loader and batch-dict contract, plus synthetic batches.

CraterDatasetCUDA mirrors /root/reference/yolo_scratch_cuda/datasets/crater_dataset_cuda.py:26-286
(decode in the workers, stretch-resize on the GPU: datasets/crater.py); collate_fn_cuda mirrors
:289-346; prepare_batch is the device transfer of train_yolo11_cuda.py:43-45; BatchAugment (datasets/augment.py)
is the training-time replacement of prepare_batch that augments on the GPU; YoloTxtDataset (datasets/yolo_txt.py)
reads images/ + labels/*.txt datasets of 1, 3 or 4 planes through the same collate and the same two launches;
datasets/letterbox.py keeps the aspect ratio instead of stretching (collate_fn_cuda(letterbox=True)) and maps boxes
between the source image and the letterboxed frame; with rect=True the frame is the batch's minimal stride-multiple
rectangle, and RectSampler (datasets/rect.py) walks a val set by aspect ratio; datasets/slicing.py plans the
overlapping full-resolution windows of sliced inference and cuts them on the GPU.
"""
from .collate import collate_fn_cuda  # noqa: F401
from .crater import CraterDatasetCUDA, max_gt_count, prepare_batch, resize_batch  # noqa: F401
from .augment import AugmentHyp, BatchAugment  # noqa: F401
from .yolo_txt import YoloTxtDataset  # noqa: F401
from .rect import RectSampler  # noqa: F401

collate_fn = collate_fn_cuda
CraterDatasetYOLO = CraterDatasetCUDA

__all__ = ["CraterDatasetCUDA", "CraterDatasetYOLO", "collate_fn_cuda", "collate_fn", "prepare_batch", "AugmentHyp",
           "BatchAugment", "YoloTxtDataset", "RectSampler"]
