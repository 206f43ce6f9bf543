"""Time the voxel-convolution path of SparseConv / SparseConvTranspose on a half-occupied 64^3 lattice (about 131 000 points,
about 13.5 pairs per row at k = 3): the max-norm search, the forward, both gradients and the list inversion, for 32 -> 32 and
8 -> 16 channels.  HIP events, medians.  The yardstick of the forward is the existing generic CConv kernel (identity mapping,
nearest neighbour, align_corners False) on the same list.  Prints one JSON line per channel pair."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import ops  # noqa: E402


def timed(fn, n=21, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def main():
    dev = torch.device("cuda:0")
    side, voxel, k = int(os.environ.get("SIDE", "64")), 0.37, 3
    rng = np.random.default_rng(0)
    zz, yy, xx = np.meshgrid(*[np.arange(side)] * 3, indexing="ij")
    cell = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)
    cell = cell[rng.random(cell.shape[0]) < 0.5]
    pos = torch.from_numpy(((cell + 0.5 + rng.uniform(-0.15, 0.15, size=cell.shape)) * voxel).astype(np.float32)).to(dev)
    n = pos.shape[0]
    radius = float(np.float32(np.float32(k * np.float32(voxel)) * np.float32(0.51)))
    extent = float(np.float32(voxel) * np.float32(k))
    search = lambda: ops.fixed_radius_search(pos, pos, radius, return_distances=False, metric="Linf")  # noqa: E731
    nns = search()
    idx, rs = nns.neighbors_index, nns.neighbors_row_splits
    t_search = timed(search)
    t_search_l2 = timed(lambda: ops.fixed_radius_search(pos, pos, radius, return_distances=False))
    t_invert = timed(lambda: ops.invert_neighbors_list(n, idx, rs))
    inv = ops.invert_neighbors_list(n, idx, rs)
    g = torch.Generator(device=dev).manual_seed(0)
    for cin, cout in ((32, 32), (8, 16)):
        W = torch.rand(k, k, k, cin, cout, device=dev, generator=g) - 0.5
        F = torch.randn(n, cin, device=dev, generator=g)
        G = torch.randn(n, cout, device=dev, generator=g)
        new = lambda: ops.sparse_conv(W, pos, voxel, [0, 0, 0], pos, F, idx, rs)  # noqa: E731
        old = lambda: ops.cconv_forward(W, pos, extent, pos, F, idx, rs, align_corners=False, coordinate_mapping="identity",  # noqa: E731
                                        interpolation="nearest_neighbor", normalize=False)
        a, b = new(), old()
        diff = float((a - b).abs().max() / b.abs().max())
        geo = (W, pos, pos, F, idx, rs, extent, [0, 0, 0])
        res = dict(points=n, pairs=int(idx.shape[0]), pairs_per_row=round(idx.shape[0] / n, 2), cin=cin, cout=cout,
                   search_linf_ms=t_search, search_l2_same_radius_ms=t_search_l2, invert_ms=t_invert,
                   forward_ms=timed(new), generic_cconv_forward_ms=timed(old),
                   generic_kernel=ops.cconv_forward(W, pos, extent, pos, F, idx, rs, align_corners=False, coordinate_mapping="identity",
                                                    interpolation="nearest_neighbor", normalize=False, name_only=True),
                   grad_filters_ms=timed(lambda: ops.sparse_gather_backward(*geo, grad_out=G, need_features=False)),
                   grad_features_ms=timed(lambda: ops.sparse_gather_backward(*geo, grad_out=G, need_filters=False, inverted=inv)),
                   max_rel_diff_to_generic=diff)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
