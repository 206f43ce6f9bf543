"""Time the forward and backward of the point-set losses on a ragged batch: ONE recording ragged call for all scenes against
the loop of un-batched recording calls, scene after scene, on the same commit (the loop is what a training batch had to run
before the ragged forms could record):

  16 scenes of 2,025 points (the scenes of tools/bench_batched_step.py: the positions against the frame one step on);
  emd_loss      looped: losses.emd_loss per scene (dmcf_emd_with_levels + dmcf_emd_backward, 62 + 4 launches per scene)
                ragged: losses.emd_loss_ragged(record=True) (dmcf_emd_ragged_with_levels + dmcf_emd_ragged_backward, 62 + 4
                launches whatever the batch)
  chamfer_loss  looped: chamfer_loss per scene (dmcf_nn_distance + dmcf_nn_distance_backward per scene)
                ragged: chamfer_loss with row splits and record=True (dmcf_nn_distance_ragged + one dmcf_nn_distance_backward)

Each measurement is ``loss(...).sum().backward()`` with the gradient taken for the predicted set, ``--inner`` times in a row,
ending device-synchronised, under a host clock; a warm-up, then the two variants alternating in one process; the median and the
range of ``--reps`` measurements, per forward + backward.  Before timing, the ragged values and gradients are checked to equal the
looped ones bit for bit.  Beside the times: the library entry points each variant calls.  Prints one JSON line and writes the
table to ``--out`` (default profiles/ragged_set_losses.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd.utils.tools.losses import emd_loss, emd_loss_ragged  # noqa: E402
from dmcf_amd.utils.tools.nn_distance import chamfer_loss  # noqa: E402
from tools.bench_batched_step import scene_items  # noqa: E402
from tools.bench_batched_valid import timed_pair  # noqa: E402
from tools.bench_batched_warm_up import library_calls  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_set_losses.md"))
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    items = scene_items(dev, args.items)
    dt = 0.0025
    tgt = [(it[0] + dt * it[1]).contiguous() for it in items]  # the target frame: one step on
    pred = [it[0].clone().requires_grad_(True) for it in items]
    T, P = torch.cat(tgt), torch.cat([p.detach() for p in pred]).requires_grad_(True)
    trs, prs = ([0] + np.cumsum([x.shape[0] for x in xs]).tolist() for xs in (tgt, pred))
    variants = {
        "emd_loss": (lambda t, p: emd_loss(t[None], p[None]), lambda: emd_loss_ragged(T, P, trs, prs, record=True)),
        "chamfer_loss": (lambda t, p: chamfer_loss(t[None], p[None]),
                         lambda: chamfer_loss(T, P, true_row_splits=trs, pred_row_splits=prs, record=True)),
    }
    res = dict(items=len(items), points_per_item=int(tgt[0].shape[0]), reps=args.reps, inner=args.inner, losses={})
    stat = lambda t: dict(median=round(float(np.median(t)), 3), min=round(float(t.min()), 3), max=round(float(t.max()), 3))  # noqa: E731
    fmt = lambda s: f"{s['median']} ({s['min']} - {s['max']})"  # noqa: E731
    rows = []
    for name, (alone, ragged_loss) in variants.items():
        def looped():
            for p in pred:
                p.grad = None
            vals = [alone(t, p) for t, p in zip(tgt, pred)]
            torch.cat(vals).sum().backward()
            return vals

        def ragged():
            P.grad = None
            val = ragged_loss()
            val.sum().backward()
            return val

        vals, val = looped(), ragged()
        assert torch.equal(torch.cat(vals).detach(), val.detach()), name
        assert torch.equal(torch.cat([p.grad for p in pred]), P.grad), name
        calls_l, calls_r = library_calls(looped), library_calls(ragged)
        many = lambda fn: (lambda: [fn() for _ in range(args.inner)])  # noqa: E731
        t_l, t_r = (np.asarray(t) / args.inner for t in timed_pair(many(looped), many(ragged), args.reps, warmup=2))
        launching = lambda c: {k: v for k, v in sorted(c.items()) if not k.endswith("_workspace_bytes")}  # noqa: E731
        r = dict(looped_ms=stat(t_l), ragged_ms=stat(t_r), library_calls_looped=launching(calls_l),
                 library_calls_ragged=launching(calls_r), bit_identical=True)
        res["losses"][name] = r
        rows.append(f"| {name} | {fmt(r['looped_ms'])} | {fmt(r['ragged_ms'])} | {sum(r['library_calls_looped'].values())} | "
                    f"{sum(r['library_calls_ragged'].values())} |\n")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# The point-set losses of a ragged batch, forward and backward: looped over the scenes against one recording call\n\n"
                f"`python tools/bench_ragged_set_losses.py` on one MI355X: {res['items']} scenes of {res['points_per_item']} points, "
                "each against its frame one step on.  Wall time of `loss(...).sum().backward()` over all scenes, the gradient taken "
                f"for the predicted set, device-synchronised ({args.inner} in a row per measurement); median (min - max) of "
                f"{args.reps} measurements, the two variants alternating in one process after a warm-up.  Looped: the un-batched "
                "recording loss called scene after scene; ragged: one call with row splits and `record=True`.  Values and "
                "gradients of the two are bit-identical (checked before timing).\n\n"
                "| loss | looped, ms | ragged, ms | library calls that enqueue, looped | ragged |\n|---|---|---|---|---|\n"
                + "".join(rows))
        for name, r in res["losses"].items():
            f.write(f"\n`{name}`, looped: {r['library_calls_looped']}; ragged: {r['library_calls_ragged']}.\n")


if __name__ == "__main__":
    main()
