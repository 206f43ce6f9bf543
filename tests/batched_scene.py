"""The small batch the row-split tests share: 3 items with 180, 1 and 260 fluid points (fixed seed) and a boundary slab each.
Items 0 and 2 occupy the same coordinates (item 2 begins with item 0's points): a lattice over the concatenation would merge
their cells.  Item 1 is a single particle far above its slab: its boundary crop keeps no row."""
import numpy as np

COUNTS = (180, 1, 260)
VOXEL = 0.05


def fluid_items(seed=7):
    """-> list of float32 [n_b, 3] arrays (z = 0: the 2-D scenes of the shipped configs)."""
    rng = np.random.RandomState(seed)
    box = rng.uniform([0.0, 0.1, 0.0], [0.6, 0.5, 0.0], size=(COUNTS[2], 3)).astype(np.float32)
    return [box[:COUNTS[0]].copy(), np.array([[0.3, 5.0, 0.0]], dtype=np.float32), box.copy()]


def slab(n=60):
    """A two-row boundary slab under the fluid box, with normals pointing up -> (positions [2n, 3], normals [2n, 3])."""
    x = np.linspace(-0.05, 0.65, n, dtype=np.float32)
    pos = np.concatenate([np.stack([x, np.full_like(x, y), np.zeros_like(x)], axis=-1) for y in (0.075, 0.05)]).astype(np.float32)
    nrm = np.tile(np.array([[0.0, 1.0, 0.0]], dtype=np.float32), (pos.shape[0], 1))
    return pos, nrm


def concat(items):
    """-> (float32 [sum n_b, 3], row splits as a list of ints)"""
    rs = [0]
    for it in items:
        rs.append(rs[-1] + it.shape[0])
    return np.concatenate(items, axis=0).astype(np.float32), rs
