"""Shared pieces of the prompt-group tests: the plans, the fixtures and torch / numpy restatements of the class maximum that do not
go through wedetect_amd/groups.py's own ``class_max``."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LVIS_EN, LVIS_ZH = "lvis_v1_class_texts.json", "lvis_v1_zh_class_texts.json"

ONE_BIN = (3, 1, 5, 2, 7, 1, 1, 4)                      # 24 prompts: one bin, eight padding rows
# eleven bins (K_pad = 352: one whole 256-column tile and a ragged one of 96).  Bin 0 ends exactly on its last class; bin 1 is a
# 32-prompt class; bin 2 holds one singleton and is closed with 31 copies of it, because bin 3 is another 32-prompt class; then a
# bin filled exactly by seven classes, two bins closed with two padding rows, four classes of eight, 32 singletons, 16 pairs, and a
# last bin with eight padding rows
K352 = (5, 27, 32, 1, 32, 3, 4, 2, 1, 6, 7, 9, 10, 10, 10, 5, 5, 5, 5, 5, 5, 8, 8, 8, 8) + (1,) * 32 + (2,) * 16 + (7, 3, 9, 1, 4)


def lvis_texts(name: str = LVIS_EN):
    with open(os.path.join(GOLDEN, name), encoding="utf-8") as f:
        return json.load(f)


def class_ranges(group_of):
    """[(first row, one past the last row)] of every class, from a non-decreasing ``group_of``."""
    go = np.asarray(group_of)
    starts = np.flatnonzero(np.r_[True, go[1:] != go[:-1]])
    return list(zip(starts.tolist(), np.r_[starts[1:], len(go)].tolist()))


def class_amax(scores, group_of):
    """torch: [..., K_pad] -> [..., G], ``amax`` over the columns of every class."""
    import torch
    return torch.stack([scores[..., a:z].amax(dim=-1) for a, z in class_ranges(group_of)], dim=-1)
