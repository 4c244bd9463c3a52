"""Inpainting masks for scripts/sample_mask_guidance.py (the role of the reference's utils/mask.py).

A mask is a [1, H, W] bool tensor: True = known pixel, False = hole. Masks are seeded per item index
(a torch CPU generator seeded with 3407 + index), so a dataset gets the same masks on every run and rank.
Types: 'center' (a central rectangle), 'rect' (random rectangles) and 'dir' (binary mask images read from a
directory with PIL, like utils/imagedir.py). The reference's 'brush' type draws strokes with PIL's ImageDraw and
is not provided.
"""
import os
from typing import Sequence, Tuple, Union

import torch

MASK_TYPES = ('center', 'rect', 'dir')
_SEED = 3407


class MaskGenerator:
    def __init__(self, mask_type: Union[str, Sequence[str]] = 'center', dir_path: str = None,
                 dir_invert_color: bool = False, center_length_ratio: Tuple[float, float] = (0.25, 0.25),
                 rect_num: Tuple[int, int] = (1, 4), rect_length_ratio: Tuple[float, float] = (0.2, 0.8)):
        types = [mask_type] if isinstance(mask_type, str) else list(mask_type)
        for t in types:
            if t == 'brush':
                raise ValueError("mask type 'brush' (PIL-drawn strokes) is not provided; use "
                                 f'one of {MASK_TYPES}')
            if t not in MASK_TYPES:
                raise ValueError(f'mask type {t} is not supported (options: {MASK_TYPES})')
        self.types = sorted(set(types))
        self.dir_invert_color = dir_invert_color
        self.center_length_ratio = center_length_ratio
        self.rect_num = rect_num
        self.rect_length_ratio = rect_length_ratio
        self.mask_paths = []
        if 'dir' in self.types:
            if dir_path is None or not os.path.isdir(os.path.expanduser(dir_path)):
                raise ValueError(f'{dir_path} is not a valid directory of mask images')
            for cur, _, files in os.walk(os.path.expanduser(dir_path)):
                self.mask_paths += [os.path.join(cur, f) for f in files
                                    if os.path.splitext(f)[1].lower() in ('.png', '.jpg', '.jpeg')]
            self.mask_paths.sort()
            if not self.mask_paths:
                raise ValueError(f'no mask images under {dir_path}')

    def sample(self, H: int, W: int, item: int) -> torch.Tensor:
        g = torch.Generator().manual_seed(_SEED + int(item))
        mask = torch.ones((1, H, W), dtype=torch.bool)
        for t in self.types:
            mask &= getattr(self, '_' + t)(H, W, g)
        return mask

    @staticmethod
    def _randint(lo: int, hi: int, g: torch.Generator) -> int:
        """An integer in [lo, hi]."""
        return int(torch.randint(lo, hi + 1, (1, ), generator=g).item())

    def _center(self, H: int, W: int, g: torch.Generator) -> torch.Tensor:
        lo, hi = self.center_length_ratio
        ratio = torch.rand((1, ), generator=g).item() * (hi - lo) + lo
        h, w = int(ratio * H), int(ratio * W)
        mask = torch.ones((1, H, W), dtype=torch.bool)
        mask[:, H // 2 - h // 2:H // 2 + h // 2, W // 2 - w // 2:W // 2 + w // 2] = False
        return mask

    def _rect(self, H: int, W: int, g: torch.Generator) -> torch.Tensor:
        lo, hi = self.rect_length_ratio
        mask = torch.ones((1, H, W), dtype=torch.bool)
        for _ in range(self._randint(*self.rect_num, g)):
            h = self._randint(int(lo * H), int(hi * H), g)
            w = self._randint(int(lo * W), int(hi * W), g)
            y = self._randint(0, H - h, g)
            x = self._randint(0, W - w, g)
            mask[:, y:y + h, x:x + w] = False
        return mask

    def _dir(self, H: int, W: int, g: torch.Generator) -> torch.Tensor:
        """A mask image (white = known, black = hole), nearest-resized to H x W."""
        import numpy as np
        from PIL import Image
        path = self.mask_paths[self._randint(0, len(self.mask_paths) - 1, g)]
        with Image.open(path) as im:   # as utils/imagedir.py reads its images
            img = torch.from_numpy(np.asarray(im.convert('L'), dtype=np.uint8).copy()).float() / 255.   # [h, w]
        ys = (torch.arange(H) * img.shape[0]) // H
        xs = (torch.arange(W) * img.shape[1]) // W
        known = img[ys][:, xs] >= 0.5
        if self.dir_invert_color:
            known = ~known
        return known[None]


class DatasetWithMask(torch.utils.data.Dataset):
    """Wraps a dataset of [C, H, W] images to return (image, mask) with the mask seeded by the item index."""

    def __init__(self, dataset, mask_type: Union[str, Sequence[str]] = 'center', **mask_kwargs):
        self.dataset = dataset
        self.mask_generator = MaskGenerator(mask_type=mask_type, **mask_kwargs)

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, item):
        image = self.dataset[item]
        image = image[0] if isinstance(image, (tuple, list)) else image
        return image, self.mask_generator.sample(int(image.shape[-2]), int(image.shape[-1]), item)
