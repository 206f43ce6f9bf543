"""Time a batch of scenes searched and convolved item by item (the loop of pipelines/simulator.py) against the same batch
concatenated and handed over in ONE call with row splits (ops.fixed_radius_search(points_row_splits=..., queries_row_splits=...),
ContinuousConv(inp_positions_row_splits=..., out_positions_row_splits=...)), for two workloads:

  ramps   16 x 2,025 points, 2-D: a 45 x 45 jittered lattice of spacing 0.01 searched at WaterRamps' radius 0.02
  box3d   8 x 50,000 points, 3-D: uniform in the unit cube, radius 0.05 (about 26 neighbours)

For each: the search with distances (points = queries), and a 32 -> 32 [4,4,4] ContinuousConv (poly6) forward plus backward
into filters and features.  HIP events around each variant, a warm-up, the two variants alternating in one process; medians.
Both variants include what they cost the host: the looped search reads one pair count per item, the batched one per call.
Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import ops  # noqa: E402
from dmcf_amd.utils.convolutions import ContinuousConv  # noqa: E402
from dmcf_amd.utils.tools.losses import get_window_func  # noqa: E402


def timed_pair(a, b, n=15, warmup=3):
    """Medians (ms) of a() and b(), measured alternately."""
    for _ in range(warmup):
        a()
        b()
    ts = ([], [])
    for _ in range(n):
        for k, fn in enumerate((a, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return round(float(np.median(ts[0])), 4), round(float(np.median(ts[1])), 4)


def workload(name, dev):
    rng = np.random.default_rng(0)
    if name == "ramps":
        g = (np.stack(np.meshgrid(np.arange(45), np.arange(45), indexing="ij"), -1).reshape(-1, 2) + 0.5) * 0.01
        items = []
        for _ in range(16):
            p = np.zeros((2025, 3), np.float32)
            p[:, :2] = g + rng.uniform(-0.003, 0.003, size=g.shape)
            items.append(p)
        return items, 0.02
    items = [rng.uniform(0, 1, size=(50000, 3)).astype(np.float32) for _ in range(8)]
    return items, 0.05


def measure(name, dev):
    items, radius = workload(name, dev)
    parts = [torch.from_numpy(p).to(dev) for p in items]
    cat = torch.cat(parts)
    rs = [0] + np.cumsum([p.shape[0] for p in parts]).tolist()
    extent = 2 * radius

    def search_looped():
        return [ops.fixed_radius_search(p, p, radius) for p in parts]

    def search_batched():
        return ops.fixed_radius_search(cat, cat, radius, points_row_splits=rs, queries_row_splits=rs)

    pairs_looped = sum(int(r.neighbors_row_splits[-1]) for r in search_looped())
    pairs_batched = int(search_batched().neighbors_row_splits[-1])
    assert pairs_looped == pairs_batched, (pairs_looped, pairs_batched)
    t_sl, t_sb = timed_pair(search_looped, search_batched)

    gen = torch.Generator(device=dev).manual_seed(0)
    layer = ContinuousConv(filters=32, kernel_size=[4, 4, 4], use_bias=False, window_function=get_window_func("poly6"), device=dev)
    layer.build(32, dev)
    layer.requires_grad_(True)
    feats = [torch.randn(p.shape[0], 32, device=dev, generator=gen).requires_grad_(True) for p in parts]
    grads = [torch.randn(p.shape[0], 32, device=dev, generator=gen) for p in parts]
    feat_cat = torch.cat([f.detach() for f in feats]).requires_grad_(True)
    grad_cat = torch.cat(grads)

    def conv_looped():
        layer.kernel.grad = None
        for p, f, g in zip(parts, feats, grads):
            f.grad = None
            (layer(f, p, p, extent) * g).sum().backward()

    def conv_batched():
        layer.kernel.grad = None
        feat_cat.grad = None
        (layer(feat_cat, cat, cat, extent, inp_positions_row_splits=rs, out_positions_row_splits=rs) * grad_cat).sum().backward()

    conv_looped()
    gw_l, gf_l = layer.kernel.grad.clone(), torch.cat([f.grad for f in feats])
    conv_batched()
    gw_b, gf_b = layer.kernel.grad.clone(), feat_cat.grad.clone()
    diff_w = float((gw_l - gw_b).abs().max() / gw_l.abs().max())
    diff_f = float((gf_l - gf_b).abs().max() / gf_l.abs().max())
    t_cl, t_cb = timed_pair(conv_looped, conv_batched)
    return dict(items=len(parts), points_per_item=parts[0].shape[0], radius=radius, pairs=pairs_batched,
                pairs_per_row=round(pairs_batched / cat.shape[0], 2), search_looped_ms=t_sl, search_batched_ms=t_sb,
                conv_fwd_bwd_looped_ms=t_cl, conv_fwd_bwd_batched_ms=t_cb, grad_filters_max_rel_diff=diff_w,
                grad_features_max_rel_diff=diff_f)


def main():
    dev = torch.device("cuda:0")
    names = os.environ.get("WORKLOADS", "ramps,box3d").split(",")
    print(json.dumps({name: measure(name, dev) for name in names}), flush=True)


if __name__ == "__main__":
    main()
