"""Detection datasets in the common `images/` + `labels/*.txt` layout, for 1-4 image planes.

    root/images/**/<stem>.<ext>      any image PIL decodes
    root/labels/**/<stem>.txt        one row per box: `cls cx cy w h`, the box normalised by the image size

The label file of an image sits under labels/ at the image's path relative to images/, with the suffix .txt.  A
missing or empty file means the image has no boxes; a row that is not five numbers with an integer class >= 0 and
a box inside the unit square raises a ValueError naming the file and the line.

As in datasets/crater.py the workers only decode: __getitem__ returns the raw uint8 image, `collate_fn_cuda(...,
channels=C)` packs the batch's bytes and one libyolomi launch (ym_resize_linear_u8c, or ym_augment_u8c under
BatchAugment) produces the fp32 (B, C, S, S) batch on the GPU.  channels == 1 decodes through crater.py's
`_gray_u8` and returns (1, h0, w0) as CraterDatasetCUDA does; 3 is RGB and 4 RGBA, returned pixel-interleaved
(h0, w0, C) as PIL yields them, with no transpose in the workers.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .crater import _gray_u8

IMG_EXTS = {".bmp", ".jpeg", ".jpg", ".png", ".tif", ".tiff", ".webp"}
_MODES = {3: "RGB", 4: "RGBA"}


def read_labels(path: Path):
    """Label file -> (boxes (n, 4) float32 cxcywh normalised, classes (n,) int64); missing or empty: n = 0."""
    boxes, labels = [], []
    if path.is_file():
        for ln, line in enumerate(path.read_text().splitlines(), 1):
            parts = line.split()
            if not parts:
                continue
            try:
                if len(parts) != 5:
                    raise ValueError("expected 5 fields")
                c = int(parts[0])
                box = [float(v) for v in parts[1:]]
                if c < 0 or not all(np.isfinite(box)) or min(box) < 0.0 or max(box) > 1.0:
                    raise ValueError("class must be >= 0 and the box inside [0, 1]")
            except ValueError as err:
                raise ValueError(f"{path}:{ln}: malformed label row {line!r} ({err}); rows are "
                                 f"`cls cx cy w h`, normalised") from None
            boxes.append(box), labels.append(c)
    if not boxes:
        return torch.zeros((0, 4), dtype=torch.float32), torch.zeros((0,), dtype=torch.long)
    return torch.tensor(boxes, dtype=torch.float32), torch.tensor(labels, dtype=torch.long)


class YoloTxtDataset(torch.utils.data.Dataset):
    """images/ + labels/*.txt dataset; items are (raw uint8 image, boxes cxcywh, classes, index) as
    CraterDatasetCUDA returns them (see the module doc for the image layout)."""

    def __init__(self, root, img_size=640, channels=3, cache_images=False):
        if channels not in (1, 3, 4):
            raise ValueError(f"YoloTxtDataset: channels must be 1 (luma), 3 (RGB) or 4 (RGBA), got {channels}")
        self.root = Path(root)
        self.img_size, self.channels, self.cache_images = img_size, int(channels), cache_images
        img_dir = self.root / "images"
        if not img_dir.is_dir():
            raise FileNotFoundError(f"YoloTxtDataset: {img_dir} is not a directory")
        files = sorted(p for p in img_dir.rglob("*") if p.is_file() and p.suffix.lower() in IMG_EXTS)
        self.samples = [{"img_path": str(p),
                         "label_path": str((self.root / "labels" / p.relative_to(img_dir)).with_suffix(".txt"))}
                        for p in files]
        self._cache, self._hw = {}, {}
        print(f"Loaded {len(self.samples)} image paths")

    def __len__(self):
        return len(self.samples)

    def load_image(self, i: int) -> np.ndarray:
        """Decoded bytes only: uint8 (h0, w0) for one plane, (h0, w0, channels) otherwise."""
        if i < 0 or i >= len(self.samples):
            raise IndexError(f"Index {i} out of range for dataset of size {len(self.samples)}")
        im = self._cache.get(i)
        if im is None:
            path = self.samples[i]["img_path"]
            if self.channels == 1:
                im = _gray_u8(path)
            else:
                from PIL import Image
                with Image.open(path) as f:
                    im = np.array(f.convert(_MODES[self.channels]), dtype=np.uint8)
            if im.size == 0 or im.shape[2:] != ((self.channels,) if self.channels > 1 else ()):
                raise ValueError(f"Invalid image shape {im.shape} for {path}")
            if self.cache_images:
                self._cache[i] = im
        return im

    def image_hw(self, i: int):
        """(h0, w0) of image i from the file's header, without decoding it; cached."""
        if i < 0 or i >= len(self.samples):
            raise IndexError(f"Index {i} out of range for dataset of size {len(self.samples)}")
        hw = self._hw.get(i)
        if hw is None:
            from PIL import Image
            with Image.open(self.samples[i]["img_path"]) as f:
                w0, h0 = f.size
            hw = self._hw[i] = (int(h0), int(w0))
        return hw

    def __getitem__(self, idx):
        im = self.load_image(idx)
        boxes, labels = read_labels(Path(self.samples[idx]["label_path"]))
        img = torch.from_numpy(np.ascontiguousarray(im))
        if self.channels == 1:
            img = img.unsqueeze(0)                                         # (1, h0, w0), as CraterDatasetCUDA
        img.img_size = self.img_size
        return img, boxes, labels, idx
