"""Training-step cost on the 1M-particle Liquid3d box (bench.py's scene, config 5): DESIGN.md section 2, "Backward pass".

  python tools/bench_backward.py [--side 100] [--steps 3] [--out bench_backward.json]

Reports
  * train_step: forward with autograd recording + weighted_mse loss + backward + Adam, ms (median of --steps after one
    warm-up) and torch.cuda.max_memory_allocated;
  * layers: per CConv / ASCC call of one training step, from HIP events around each launch (ops.timer): the forward kernel,
    the neighbour-list inversion and the backward (both gradients);
  * split: for a 24-channel 4x4x4 layer on the box's own list at the second scale's radius (hundreds of neighbours per
    row, like the two 24-channel layers of the network), the forward, the inversion, the input-feature gradient alone and
    the filter gradient alone;
  * lattice: the s1 -> s1 and s1 -> s2 lattice layers of the box (grid_pos at 2x and 4x the voxel size, extents 0.4 and
    0.8, 8 -> 8 channels), forward plus both gradients in the stencil form (ops.lattice_conv, ops.lattice_conv_backward:
    no list) against the neighbour-list route (search + inversion + forward + ops.cconv_backward);
  * scatter: the particles -> s2 (24 -> 4, R = 0.4) and particles -> s1 (24 -> 8, R = 0.2) layers of the box, both gradients on
    route A (forward-list search + ops.invert_neighbors_list + ops.cconv_backward) against route B (transposed search +
    ops.cconv_scatter_backward), alternating inside the process: medians of --reps repeats and the spread of each.
--lattice-form / --scatter-form record the training step with model.record_lattice_form(True) / record_scatter_form(True);
--sections picks what runs (train,layers,split,lattice,scatter; default all)."""
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


def timed(fn, n=5):
    fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


def lattice_layers(cfg, pos, dev):
    """The two longest-row lattice layers of the box, stencil route against neighbour-list route (ms, medians)."""
    from dmcf_amd import lattice
    vs = np.float32(cfg["voxel_size"])
    s1 = ops.grid_pos(pos, vs * 2, centralize=True)
    s2 = ops.grid_pos(pos, vs * 4, centralize=True)
    res = {}
    for tag, A, B, extent in (("s1->s1", s1, s1, 0.4), ("s1->s2", s1, s2, 0.8)):
        cin = cout = 8
        rng = np.random.default_rng(0)
        n_in, n_out = A.shape[0], B.shape[0]
        F = torch.from_numpy(rng.normal(size=(n_in, cin)).astype(np.float32)).to(dev)
        W = torch.from_numpy(rng.uniform(-0.1, 0.1, size=(4, 4, 4, cin, cout)).astype(np.float32)).to(dev)
        G = torch.from_numpy(rng.normal(size=(n_out, cout)).astype(np.float32)).to(dev)
        lp = lattice.pair(A, B, extent)
        vmin, vdim, parts = lp.plan(ops, extent, dev)
        table, tmin = lp.out.table(), lp.out.minp
        kw = dict(inp_step=int(lp.ratio), window="poly6")
        row = dict(n_in=n_in, n_out=n_out, offsets=int(ops.lattice_offsets(lp.inp.voxel, 0.5 * extent, dev).shape[0]))
        row["stencil_forward"] = timed(lambda: ops.lattice_conv(W, lp.inp.volume(F, vmin, vdim), vmin, table, tmin, n_out,
                                                                lp.inp.voxel, extent, **kw))
        vol = lp.inp.volume(F, vmin, vdim)
        row["stencil_backward"] = timed(lambda: ops.lattice_conv_backward(W, vol, vmin, table, tmin, n_out, lp.inp.voxel, extent, G, **kw))
        radius = 0.5 * extent
        row["list_search"] = timed(lambda: ops.fixed_radius_search(A, B, radius, return_distances=False))
        nns = ops.fixed_radius_search(A, B, radius, return_distances=False)
        idx, rs = nns.neighbors_index, nns.neighbors_row_splits
        row["pairs"] = int(rs[-1])
        row["list_forward"] = timed(lambda: ops.cconv_forward(W, B, extent, A, F, idx, rs, window="poly6", row_length_hint=2))
        row["list_invert"] = timed(lambda: ops.invert_neighbors_list(n_in, idx, rs))
        inv = ops.invert_neighbors_list(n_in, idx, rs)
        row["list_grad_inp_features"] = timed(lambda: ops.cconv_backward(W, B, extent, A, F, idx, rs, G, window="poly6",
                                                                         need_filters=False, inverted=inv))
        row["list_grad_filters"] = timed(lambda: ops.cconv_backward(W, B, extent, A, F, idx, rs, G, window="poly6",
                                                                    need_features=False))
        row["stencil_total_ms"] = row["stencil_forward"]["ms_median"] + row["stencil_backward"]["ms_median"]
        row["list_total_ms"] = sum(row[k]["ms_median"] for k in ("list_search", "list_forward", "list_invert",
                                                                  "list_grad_inp_features", "list_grad_filters"))
        res[tag] = row
        print(json.dumps({f"lattice {tag}": row}), flush=True)
    return res


def split_gradients(cfg, pos, dev):
    """The two gradients of one wide-radius 24-channel layer, separately."""
    n = pos.shape[0]
    radius = float(np.float32(cfg["particle_radii"][1]))
    nns = ops.fixed_radius_search(pos, pos, radius, return_distances=False)
    idx, rs = nns.neighbors_index, nns.neighbors_row_splits
    pairs = int(rs[-1])
    split = dict(pairs=pairs, radius=radius)
    for cin, cout in ((24, 16), (24, 32)):
        rng = np.random.default_rng(0)
        F = torch.from_numpy(rng.normal(size=(n, cin)).astype(np.float32)).to(dev)
        W = torch.from_numpy(rng.uniform(-0.1, 0.1, size=(4, 4, 4, cin, cout)).astype(np.float32)).to(dev)
        G = torch.from_numpy(rng.normal(size=(n, cout)).astype(np.float32)).to(dev)
        kw = dict(window="poly6", row_length_hint=2)
        out = torch.empty(n, cout, device=dev)
        inv = ops.invert_neighbors_list(n, idx, rs)
        gw = torch.empty_like(W)
        gf = torch.empty_like(F)
        row = dict(kernel=ops.cconv_forward(W, pos, 2 * radius, pos, F, idx, rs, name_only=True, **kw))
        row["forward"] = timed(lambda: ops.cconv_forward(W, pos, 2 * radius, pos, F, idx, rs, out=out, **kw))
        row["invert"] = timed(lambda: ops.invert_neighbors_list(n, idx, rs))
        row["grad_inp_features"] = timed(lambda: ops.cconv_backward(W, pos, 2 * radius, pos, F, idx, rs, G, window="poly6",
                                                                    need_filters=False, inverted=inv, grad_inp_features=gf))
        row["grad_filters"] = timed(lambda: ops.cconv_backward(W, pos, 2 * radius, pos, F, idx, rs, G, window="poly6",
                                                               need_features=False, grad_filters=gw))
        split[f"{cin}->{cout}"] = row
        print(json.dumps({f"split {cin}->{cout}": row}), flush=True)
    return split


def _spread(ts):
    """Median and spread (max - min; the 10 % .. 90 % range beside it) of a list of times."""
    return dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)),
                ms_spread=float(np.max(ts) - np.min(ts)), ms_p10_p90=float(np.percentile(ts, 90) - np.percentile(ts, 10)))


def scatter_layers(cfg, pos, dev, reps=20):
    """The two particles -> lattice layers with few output channels: both gradients through the list route (A) and through the
    input-stationary route (B), the two alternating, HIP events around each route and around its parts."""
    vs = np.float32(cfg["voxel_size"])
    res = {}
    for tag, stride, cin, cout, radius in (("s0->s2", 4, 24, 4, 0.4), ("s0->s1", 2, 24, 8, 0.2)):
        B = ops.grid_pos(pos, vs * stride, centralize=True)
        extent = float(np.float32(2) * np.float32(radius))
        radius = float(np.float32(0.5) * np.float32(extent))
        rng = np.random.default_rng(0)
        n_in, n_out = pos.shape[0], B.shape[0]
        F = torch.from_numpy(rng.normal(size=(n_in, cin)).astype(np.float32)).to(dev)
        W = torch.from_numpy(rng.uniform(-0.1, 0.1, size=(4, 4, 4, cin, cout)).astype(np.float32)).to(dev)
        G = torch.from_numpy(rng.normal(size=(n_out, cout)).astype(np.float32)).to(dev)

        def marks(k):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(k)]
            return ev

        def route_a():
            ev = marks(4)
            ev[0].record()
            nns = ops.fixed_radius_search(pos, B, radius, return_distances=False)
            idx, rs = nns.neighbors_index, nns.neighbors_row_splits
            ev[1].record()
            inv = ops.invert_neighbors_list(n_in, idx, rs)
            ev[2].record()
            gw, gf = ops.cconv_backward(W, B, extent, pos, F, idx, rs, G, window="poly6", inverted=inv)
            ev[3].record()
            return ev, (gw, gf), int(idx.shape[0])

        def route_b():
            ev = marks(3)
            ev[0].record()
            tl = ops.fixed_radius_search(B, pos, radius, return_distances=False)
            ev[1].record()
            gw, gf = ops.cconv_scatter_backward(W, B, extent, pos, F, tl.neighbors_index, tl.neighbors_row_splits, None, G, window="poly6")
            ev[2].record()
            return ev, (gw, gf), int(tl.neighbors_index.shape[0])

        _, ga, pairs_a = route_a()
        _, gb, pairs_b = route_b()
        torch.cuda.synchronize()
        row = dict(n_in=n_in, n_out=n_out, cin=cin, cout=cout, pairs=pairs_a, pairs_transposed=pairs_b,
                   max_rel_diff_filters=float((ga[0] - gb[0]).abs().max() / ga[0].abs().max()),
                   max_rel_diff_features=float((ga[1] - gb[1]).abs().max() / ga[1].abs().max()))
        del ga, gb
        ta, tb = [], []
        for _ in range(reps):
            ea, _, _ = route_a()
            torch.cuda.synchronize()
            ta.append([ea[i].elapsed_time(ea[i + 1]) for i in range(3)])
            eb, _, _ = route_b()
            torch.cuda.synchronize()
            tb.append([eb[i].elapsed_time(eb[i + 1]) for i in range(2)])
        ta, tb = np.asarray(ta), np.asarray(tb)
        row["A_total"], row["B_total"] = _spread(ta.sum(1)), _spread(tb.sum(1))
        for k, name in enumerate(("A_search", "A_invert", "A_backward")):
            row[name] = _spread(ta[:, k])
        for k, name in enumerate(("B_search", "B_backward")):
            row[name] = _spread(tb[:, k])
        row["B_wins"] = bool(row["A_total"]["ms_median"] - row["B_total"]["ms_median"] >
                             max(row["A_total"]["ms_spread"], row["B_total"]["ms_spread"]))
        res[tag] = row
        print(json.dumps({f"scatter {tag}": row}), flush=True)
        del B, F, G
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lattice-form", action="store_true")
    ap.add_argument("--scatter-form", action="store_true")
    ap.add_argument("--reps", type=int, default=20, help="repeats of each route in the scatter section")
    ap.add_argument("--sections", default="train,layers,split,lattice,scatter")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backward needs a GPU")
    dev = torch.device("cuda:0")
    cfg = dict(configs.LIQUID3D)
    cfg["loss"] = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025, pre_scale=0.025)}
    model = getattr(models, cfg["name"])(**cfg)
    tc.load_into_model(model, dict(np.load(os.path.join(ROOT, "tests", "golden", "liquid3d_weights.npz"))), device=dev)
    data = scenes.model_inputs(scenes.box_scene(args.side), device=dev)
    with torch.no_grad():
        model(data)
    model.requires_grad_(True)
    model.record_lattice_form(args.lattice_form)
    model.record_scatter_form(args.scatter_form)
    sections = set(args.sections.split(","))
    opt, sched = model.get_optimizer({"lr_boundaries": [1000], "lr_values": [1e-4, 1e-5]})
    target = data[0] + model.timestep * data[1]

    def train_step():
        pos2, vel2 = model(data)
        loss = model.loss([pos2, vel2], ([data[0]], target, data[0], 0))["weighted_mse"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()

    result = dict(points=int(data[0].shape[0] + data[4].shape[0]), fluid=int(data[0].shape[0]), lattice_form=bool(args.lattice_form),
                  scatter_form=bool(args.scatter_form))
    if "train" in sections:
        train_step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        result["train_step"] = timed(train_step, args.steps)
        result["train_step"]["max_memory_allocated_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
        print(json.dumps({"train_step": result["train_step"]}), flush=True)
        with torch.no_grad():
            result["inference_step"] = timed(lambda: model(data), args.steps)
        print(json.dumps({"inference_step": result["inference_step"]}), flush=True)

    if "layers" in sections:
        # per-call breakdown of one training step
        ops.timer = ops.LaunchTimer()
        train_step()
        torch.cuda.synchronize()
        recs = ops.timer.results()
        ops.timer = None
        layers = [dict(kind=k, ms=ms, **m) for k, m, ms in recs]
        result["layers"] = layers
        tot = {}
        for r in layers:
            tot[r["kind"]] = tot.get(r["kind"], 0.0) + r["ms"]
        result["layer_totals_ms"] = tot
        print(json.dumps({"layer_totals_ms": tot}), flush=True)

    pos = torch.cat([data[0], data[4]]).contiguous()
    if "split" in sections:
        result["split"] = split_gradients(cfg, pos, dev)
    if "lattice" in sections:
        result["lattice"] = lattice_layers(cfg, data[0], dev)
    if "scatter" in sections:
        del model, opt, sched
        torch.cuda.empty_cache()
        result["scatter"] = scatter_layers(cfg, pos, dev, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
