"""Writes a tiny synthetic TRAIN split in dataset/prepare_data.py's layout: img/<idx>.jpg, mask/<idx>.jpg, dense/<idx>.jpg (256x256) and
anno/<idx>.pkl.  The img and anno files are those of fake_split.write_split; the mask holds a left (G > R) and a right (R > G) blob on black,
the dense map smooth colours inside them."""
import os

import numpy as np

from fake_split import write_split


def write_train_split(root, n, seed=0, size=256):
    from PIL import Image
    write_split(root, n, split='train', seed=seed, size=size)
    rng = np.random.RandomState(seed + 1000)
    yy, xx = np.mgrid[0:size, 0:size]
    for kind in ('mask', 'dense'):
        os.makedirs(os.path.join(root, 'train', kind), exist_ok=True)
    for i in range(n):
        cl, cr = rng.uniform(60, 110, 2), rng.uniform(140, 200, 2)
        left = (xx - cl[0]) ** 2 + (yy - cl[1]) ** 2 < rng.uniform(30, 50) ** 2
        right = (xx - cr[0]) ** 2 + (yy - cr[1]) ** 2 < rng.uniform(30, 50) ** 2
        mask = np.zeros((size, size, 3), np.uint8)
        mask[left] = (0, 200, 40)                      # BGR: G > R -> left
        mask[right] = (0, 40, 200)                     # R > G -> right
        dense = np.zeros((size, size, 3), np.float64)
        for c in range(3):
            dense[..., c] = 127 + 120 * np.sin(xx / (13.0 + c + i)) * np.cos(yy / (9.0 + c))
        dense[~(left | right)] = 0
        for kind, a in (('mask', mask), ('dense', dense)):
            Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)[:, :, ::-1]).save(os.path.join(root, 'train', kind, '%d.jpg' % i), quality=95)
