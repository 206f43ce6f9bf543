"""PointNet's layer and model on the 1M-particle 2-D box (1000 x 1000 fluid particles at spacing 0.005, R = 0.01, a
boundary shell): DESIGN.md section 4.8.

  python tools/bench_pointnet.py [--side 1000] [--reps 10] [--out bench_pointnet.json]

Reports (HIP events, median of --reps after a warm-up)
  * layers: per layer of the shipped config, the fused forward (dmcf_neighbor_dense_forward), the torch composition of the
    same layer in this process (addmm -> index_select -> index_add_ segment sum -> residual add), the backward
    (dmcf_neighbor_dense_backward: input gradient, dW and db) and the shared inversion of the list;
  * the inference step and the training step (forward recording, weighted_mse, backward) of the whole model;
  * launches: the kernel launches of one inference step on the 60 x 60 box with a shell of bench.py --config wbcsph."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import models, ops  # noqa: E402
from dmcf_amd.utils import tf_checkpoint as tc  # noqa: E402
from tools import configs, scenes  # noqa: E402


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


def seeded_model(dev, **over):
    cfg = dict(configs.POINTNET2D, **over)
    m = models.PointNet(**cfg)
    rng = np.random.default_rng(0)
    widths = [7] + m.layer_channels
    w = {}
    for i in range(len(m.layer_channels)):
        w[f"model/denses/{i}/kernel"] = (rng.normal(size=(widths[i], widths[i + 1])) / np.sqrt(widths[i])).astype(np.float32)
        w[f"model/denses/{i}/bias"] = rng.normal(scale=0.1, size=widths[i + 1]).astype(np.float32)
    tc.load_into_model(m, w, device=dev)
    return m


def torch_layer(x, W, b, idx, rs_rows, n_out, residual):
    """The reference's order as a torch composition: Dense, gather, segment sum, residual."""
    d = torch.addmm(b, torch.relu(x), W)
    ok = idx < d.shape[0]
    g = d.index_select(0, torch.where(ok, idx, torch.zeros_like(idx))) * ok[:, None]
    s = torch.zeros(n_out, W.shape[1], device=x.device).index_add_(0, rs_rows, g)
    return s + residual if residual is not None else s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet needs a GPU")
    dev = torch.device("cuda:0")
    res = {"side": args.side}
    model = seeded_model(dev, loss={"weighted_mse": dict(typ="weighted_mse", fac=1000.0, gamma=0.5, neighbor_scale=0.0625)})
    data = scenes.model_inputs(scenes.box_scene(args.side, h=0.005, dim=2, vel_std=0.05), device=dev, grav=[0.0, -9.81, 0.0])
    with torch.no_grad():
        model(data, training=False)
    idx, rs = model.neighbors_index, model.neighbors_row_splits
    n_all = rs.shape[0] - 1
    P = int(rs[-1].item())
    res.update(n_fluid=int(data[0].shape[0]), n_all=int(n_all), pairs=P)
    rows = torch.repeat_interleave(torch.arange(n_all, device=dev), torch.diff(rs))
    idx_l = idx[:P].long()
    # the layer inputs of one step
    with torch.no_grad():
        xs = [model.inp_feats]
        for dense in model.denses[:-1]:
            r = xs[-1] if dense.units == xs[-1].shape[1] else None
            xs.append(ops.neighbor_dense(xs[-1], dense.kernel, dense.bias, idx, rs, residual=r))
    inv = {}
    res["inversion"] = timed(lambda: inv.__setitem__("v", ops.invert_neighbors_list(n_all, idx, rs)), args.reps)
    layers = []
    for i, (dense, x) in enumerate(zip(model.denses, xs)):
        W, b = dense.kernel, dense.bias
        r = x if dense.units == x.shape[1] else None
        e = dict(layer=i, cin=int(W.shape[0]), cout=int(W.shape[1]), residual=r is not None, n_in=int(x.shape[0]))
        with torch.no_grad():
            e["fused_forward"] = timed(lambda: ops.neighbor_dense(x, W, b, idx, rs, residual=r), args.reps)
            e["torch_composition"] = timed(lambda: torch_layer(x, W, b, idx_l, rows, n_all, r), args.reps)
            y, s, c = ops._nd_forward(x, W, b, idx, rs, None, True, r, None, record=True)
            G = torch.randn_like(y)
            e["backward"] = timed(lambda: ops.neighbor_dense_backward(x, W, G, s, c, inverted=inv["v"], need_x=i > 0), args.reps)
            ref = torch_layer(x, W, b, idx_l, rows, n_all, r)
            e["max_abs_diff_vs_torch"] = float((y - ref).abs().max())
        e["speedup_vs_torch"] = e["torch_composition"]["ms_median"] / e["fused_forward"]["ms_median"]
        e["fwd_plus_bwd_over_fwd"] = (e["fused_forward"]["ms_median"] + e["backward"]["ms_median"]) / e["fused_forward"]["ms_median"]
        layers.append(e)
        del y, s, c, G
    res["layers"] = layers
    with torch.no_grad():
        res["inference_step"] = timed(lambda: model(data, training=False), args.reps)
    target = data[0] + 0.0025 * data[1]
    model.requires_grad_(True)

    def train_step():
        model.zero_grad(set_to_none=True)
        out = model(data, training=True)
        model.loss(out, (data, target, None, 0))["weighted_mse"].backward()

    torch.cuda.reset_peak_memory_stats()
    res["training_step"] = timed(train_step, max(3, args.reps // 2))
    res["training_step"]["max_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    model.requires_grad_(False)
    # launches of one inference step on the small box
    small = scenes.model_inputs(scenes.box_scene(60, h=0.005, dim=2), device=dev, grav=[0.0, -9.81, 0.0])
    with torch.no_grad():
        model(small, training=False)
    ops.timer = ops.LaunchTimer()
    with torch.no_grad():
        model(small, training=False)
    torch.cuda.synchronize()
    kinds = [(k, m.get("kernel")) for k, m, _ in ops.timer.results()]
    ops.timer = None
    res["small_step_launches"] = dict(neighbor_dense=sum(1 for k, _ in kinds if k == "neighbor_dense"), all=kinds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
