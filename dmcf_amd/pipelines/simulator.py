"""Simulator -- mirror of the inference surface of the reference's ``pipelines/simulator.py:37-109``.

``run_inference(inputs)`` (simulator.py:57-71) takes a list of per-scene input lists
``[pos, vel, acc|None, feats|None, box, box_normals]`` and returns ``[pos', vel'] + inputs[2:]`` per scene so
the result is fed back verbatim; ``run_rollout(inputs, timesteps)`` (:73-109) loops it.  The reference has
no ``step()``; it is provided as an alias because BASELINE.json names that surface.

``run_test`` (:111-165) writes the rollouts of the test split; ``run_valid`` (:167-285) rolls out the validation split and
computes the reference's metrics (MSE, Chamfer both ways, density errors, approximate-match EMD, velocity-histogram KL, the
one-step MSE) with the nearest-neighbour and EMD kernels of dmcf_amd/csrc/metrics.hip.  ``run_train`` (:287-518) is the
training loop: ``train_step`` (the reference's ``train(data, time_w, it, max_err, max_dens_err)``) warms every sample up
on the inference path, records the time-weighted window, back-propagates and applies utils/tools/losses.KerasAdam
(dmcf_adam_step); the outer loop follows the window / warm-up / iteration schedules, writes checkpoints with their Adam
state (utils/tf_checkpoint.CheckpointManager) and validates and tests after every epoch.  The number of particles may
change between steps (run_sample.py:173-177 adds inflow), so nothing here assumes a fixed N.  Opt-in batched forms (pipeline
keys, all default false): ``train_batched`` and ``warm_up_batched`` for the training window and its warm-up, ``valid_batched``
for run_valid -- ``run_rollout_batched`` advances all scenes with one ``model.step_batched`` per time step and
``valid_losses_batched`` evaluates a frame of all scenes at once (one dmcf_nn_distance_ragged call for the Chamfer metric, one
dmcf_emd_ragged call for the EMD, one dmcf_hist_pair_ragged call for the two velocity-histogram KLs).
``train_set_losses`` (default none; needs ``train_batched``) adds correspondence-free Chamfer / EMD terms to the training
window, each ONE recording ragged call per window step over all samples.
"""
import logging
import os
import time
from datetime import datetime

import numpy as np
import torch

from ..utils.config import Config
from .. import ops
from ..utils.convolutions import neighbor_cache

log = logging.getLogger(__name__)


# 1M fluid + 0.12M boundary particles peak at 16 GB of live buffers and ~45 GB of pool once the lists have grown (DESIGN.md
# section 4.1): 40 KiB per point
RESERVE_BYTES_PER_POINT = 40 * 1024

SET_LOSSES = ("chamfer", "emd")  # the names pipeline key train_set_losses takes


def reserve_for_scene(reserve_gib, n_points, device):
    """The ``reserve_gib`` rule of Simulator / ShardedSimulator for a scene of ``n_points`` particles (fluid + boundary): "auto" =
    RESERVE_BYTES_PER_POINT each, at most an eighth of the device, at least 0.25 GiB.  Returns what ops.reserve_device_memory reports (0.0 when nothing was asked for)."""
    gib = reserve_gib
    if gib and device is not None and torch.device(device).type == "cuda":
        # torch's allocator serves requests up to 1 MB from 2 MB segments of their own ("small pool"): row splits, counts,
        # headers, the 2-D scenes' whole lists.  That pool grows one hipMalloc at a time whenever a step needs one block more
        # than any step before it (round 3: six such steps in the 3200-step rollout) -- hold 64 MB of it from the start.
        small = [torch.empty(1 << 20, dtype=torch.uint8, device=device) for _ in range(64)]
        del small
        # ... and load the code of the library kernels a rollout may meet late: grid_pos's sort-based form (torch.unique +
        # argsort, taken once stray particles make the lattices' bounding box too sparse for a dense cell table) cost the
        # 100k dam break 300 ms in the step that first needed it
        from ..utils.tools.losses import _unique_first_occurrence
        _unique_first_occurrence(torch.arange(8, dtype=torch.int64, device=device) % 3)
    if gib == "auto":
        gib = n_points * RESERVE_BYTES_PER_POINT / 2 ** 30
        gib = min(gib, torch.cuda.mem_get_info(device)[1] / 2 ** 30 / 8)  # (total device memory)
        gib = max(gib, 0.25)  # (the 2-D scenes: their lists are a few MB, but grow with every particle that leaves the tank)
        log.info("reserve_gib='auto': %.2f GiB of device memory go to the caching allocator's pool before the first step", gib)
    return ops.reserve_device_memory(float(gib), device) if gib else 0.0


class steady_steps:
    """``with steady_steps(): for ...: sim.step(...)`` -- Python's cyclic garbage collector off for the duration of a rollout
    loop (the young generation is collected by hand every ``every`` steps).  A step of the 2-D models is ~5 ms of host work
    (40+ launches per layer stack); a generation-2 collection in the middle of one is what the rollouts' p99 showed
    (WBC-SPH, 3200 steps: p99 / median 1.2 - 1.55 with the collector running, 1.22 without, tools/long_rollout.py).
    ``Simulator.run_rollout`` runs inside one.  The switch is process wide (other threads see the collector off as well) for
    the duration of the ``with`` block."""

    def __init__(self, every=256):
        self.every, self.n = int(every), 0

    def __enter__(self):
        import gc
        self.gc, self.was = gc, gc.isenabled()
        gc.collect()
        gc.disable()
        return self

    def tick(self, full=False):
        """Once per step.  ``full``: a whole collection now (a step was repeated: the exception's traceback may hold device
        tensors in a cycle); otherwise the young generation every ``every`` steps and everything every 16 x ``every`` -- cycles
        that hold device buffers (closures of the neighbour lists, tracebacks) must not live until the rollout ends."""
        self.n += 1
        if full or self.n % (16 * self.every) == 0:
            self.gc.collect()
        elif self.n % self.every == 0:
            self.gc.collect(0)

    def __exit__(self, *exc):
        if self.was:
            self.gc.enable()
        return False


class WarmUpExits:
    """The host side of the batched warm-up (Simulator.warm_up_batched): which samples are still warming up, and the early
    exits of simulator.py:325-368 decided per sample exactly as the per-sample loop decides them -- ``max_err`` first, its
    break skipping the density test; ``p > 0 and err > prev and err > limit``; a previous error updated only when its test
    was reached.  No device, no tensors."""

    def __init__(self, pre, max_err=None, max_dens_err=None):
        self.pre = [int(k) for k in pre]
        self.max_err, self.max_dens_err = max_err, max_dens_err
        self.prev_err = [0.0] * len(self.pre)
        self.prev_dens_err = [0.0] * len(self.pre)
        self.left = [None] * len(self.pre)  # the iteration at which the sample broke out

    def active(self, p):
        """The samples that take step ``p``: ``pre > p`` and not left."""
        return [bi for bi, k in enumerate(self.pre) if k > p and self.left[bi] is None]

    def accept(self, p, bi, err=None, dens_err=None):
        """Sample ``bi``'s errors after step ``p`` -> True: the step's state is taken; False: the sample leaves with the
        state from before the step."""
        if self.max_err is not None:
            if p > 0 and err > self.prev_err[bi] and err > self.max_err:
                self.left[bi] = p
                return False
            self.prev_err[bi] = err
        if self.max_dens_err is not None:
            if p > 0 and dens_err > self.prev_dens_err[bi] and dens_err > self.max_dens_err:
                self.left[bi] = p
                return False
            self.prev_dens_err[bi] = dens_err
        return True

    def pres(self):
        """What the loop hands on: the iteration of the break, else the last loop index pre - 1 (0 for pre == 0)."""
        return [max(k - 1, 0) if at is None else at for k, at in zip(self.pre, self.left)]


def valid_frames(lengths, eval_stride=1):
    """The host bookkeeping of the batched validation (Simulator.valid_losses_batched): scene i has ``lengths[i]`` frames and
    run_valid evaluates its frames t = 1 .. lengths[i] - 1 with ``t % eval_stride == 0``.  -> [(t, [the scenes that have an
    evaluated frame t, ascending])] in ascending t, frames nobody has left out.  No device, no tensors."""
    eval_stride = int(eval_stride)
    if eval_stride < 1:
        raise ValueError(f"eval_stride must be >= 1, got {eval_stride}")
    frames = []
    for t in range(eval_stride, max((int(k) for k in lengths), default=0), eval_stride):
        frames.append((t, [i for i, k in enumerate(lengths) if t < int(k)]))
    return frames


class Simulator:
    def __init__(self, model, dataset=None, name="Simulator", main_log_dir="./logs/", device="cuda", split="train",
                 reserve_gib=None, **kwargs):
        """``reserve_gib`` (not in the reference; a ``pipeline:`` key like the others, OFF unless asked for): device memory handed
        to torch's caching allocator as one block before the first step (ops.reserve_device_memory), so that the multi-GB
        neighbour-list buffers of a large scene -- and the bigger ones it grows into -- never wait for a hipMalloc in the middle
        of a rollout.  "auto" = RESERVE_BYTES_PER_POINT per particle (fluid + boundary) of the first scene, at most an EIGHTH of
        the device (43 GiB would be the rule's figure for 1M particles: 36 GiB on a 288 GB part), logged when taken; a number =
        that many GiB; 0 / None (the default) = none -- the library itself never allocates device memory (INTEGRATION.md
        section 4), and a caller who did not ask does not lose a slice of the device to this module either.  bench.py asks for
        "auto" and reports what it got (``scene_state.reserved_gib``)."""
        self.cfg = Config(dict(kwargs, name=name, main_log_dir=main_log_dir, device=device, split=split, reserve_gib=reserve_gib))
        self.name = name
        self.model = model
        self.dataset = dataset
        if device in ("gpu", "cuda"):
            device = "cuda"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the DMCF hot path runs on the GPU only (no CPU fallback)")
        self.timing = []
        self.reserve_gib = reserve_gib
        self.reserved_gib = None  # what the first step took from the device (None: not asked yet)
        self._slot0 = 0  # scene slot of inputs[0] (run_rollout feeds its scenes one at a time)
        self.repeated_steps = 0  # steps repeated with exact buffer sizes after a NeighborCapacityExceeded
        # base_pipeline.py:46-63: <main_log_dir | output_dir>/<Model>_<dataset>_<version>
        tag = "_".join([type(model).__name__, dataset.name if dataset is not None and hasattr(dataset, "name") else "",
                        str(kwargs.get("version", ""))])
        self.cfg.logs_dir = os.path.join(main_log_dir, tag)
        self.cfg.out_dir = os.path.join(kwargs.get("output_dir", "./output"), tag)
        if split == "train" and kwargs.get("restart"):  # base_pipeline.py:54-65 (the train split only here)
            import shutil
            for d in (self.cfg.logs_dir, self.cfg.out_dir):
                if os.path.exists(d):
                    shutil.rmtree(d)
        self.optimizer = None
        self.set_losses = self._set_losses()

    def _set_losses(self):
        """Pipeline key ``train_set_losses`` (default none): a mapping from "chamfer" / "emd" to a factor, e.g. ``{chamfer: 1.0,
        emd: 0.1}`` -> [(name, factor)] in the mapping's order.  Every window step of a ``train_batched`` window then adds
        ``factor * loss`` of the samples' new positions against their target frames as one more column per name of the loss
        vector.  An unknown name is a ValueError, the key without ``train_batched`` a NotImplementedError (the per-sample window
        has no batch to make one call for) -- both here, before anything runs."""
        conf = self.cfg.get("train_set_losses", None)
        if not conf:
            return []
        terms = [(str(k), float(v)) for k, v in dict(conf).items()]
        for name, _ in terms:
            if name not in SET_LOSSES:
                raise ValueError(f"train_set_losses: unknown loss {name!r} (one of {', '.join(SET_LOSSES)})")
        if not self.cfg.get("train_batched", False):
            raise NotImplementedError("train_set_losses needs train_batched: the terms are one ragged call per window step")
        return terms

    def loss_keys(self):
        """The names of the entries of the training loss vector: the model's, then those of ``train_set_losses``."""
        return list(self.model.loss_keys()) + [name for name, _ in self.set_losses]

    def _set_loss_columns(self, pos2, rs, targets):
        """[batch, len(train_set_losses)]: ``factor * loss`` per sample and configured name, every name ONE recording ragged
        call over all samples: their rows of ``pos2`` (row splits ``rs``) against ``targets`` (one frame per sample)."""
        from ..utils.tools.losses import emd_loss_ragged
        from ..utils.tools.nn_distance import chamfer_loss
        tgt = torch.cat(targets, dim=0)
        trs = [0]
        for x in targets:
            trs.append(trs[-1] + x.shape[0])
        cols = []
        for name, fac in self.set_losses:
            if name == "chamfer":
                value = chamfer_loss(tgt, pos2, true_row_splits=trs, pred_row_splits=rs, record=True)
            else:
                value = emd_loss_ragged(tgt, pos2, trs, rs, record=True)
            cols.append(fac * value)
        return torch.stack(cols, dim=1)

    def _to_device(self, x):
        if x is None:
            return None
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return x.to(self.device, dtype=torch.float32)

    def _reserve(self, inputs):
        """Once, before the first step: see ``reserve_gib`` in __init__."""
        n = max((int(s[0].shape[0]) + (int(s[4].shape[0]) if s[4] is not None else 0) for s in inputs), default=0)
        self.reserved_gib = reserve_for_scene(self.reserve_gib, n, self.device)

    @torch.no_grad()
    def run_inference(self, inputs):
        """simulator.py:57-71."""
        if self.reserved_gib is None:
            self._reserve(inputs)
        results = []
        for bi in range(len(inputs)):
            try:
                with neighbor_cache(estimate=True, key=(id(self.model), bi + self._slot0)):
                    pos, vel = self.model(inputs[bi], training=False)
            except ops.NeighborCapacityExceeded:
                # a neighbour list grew by more than the slack since the previous step: repeat with exact sizes
                self.repeated_steps += 1
                with neighbor_cache(estimate=False, key=(id(self.model), bi + self._slot0)):
                    pos, vel = self.model(inputs[bi], training=False)
            results.append([pos, vel] + list(inputs[bi][2:]))
        return results

    def step(self, inputs):
        """Alias of :meth:`run_inference` (one simulated time step)."""
        return self.run_inference(inputs)

    @torch.no_grad()
    def run_rollout(self, inputs, timesteps=2):
        """simulator.py:73-109.  ``inputs``: list of dicts with [T,N,3] arrays ``pos, vel, grav, box,
        box_normals`` (frame 0 is used), as produced by get_rollout (dataset_reader_physics.py:410-456)."""
        inputs = [[self._to_device(data["pos"][0]), self._to_device(data["vel"][0]),
                   self._to_device(data["grav"][0]) if data.get("grav") is not None and data["grav"][0] is not None
                   else None, None, self._to_device(data["box"][0]), self._to_device(data["box_normals"][0])]
                  for data in inputs]
        results = [[] for _ in range(len(inputs))]
        self.run_inference(inputs[:1])  # "dummy init": builds the lazily created weights (simulator.py:94)
        timing = []
        for i in range(len(inputs)):
            results[i].append(inputs[i])
        with steady_steps() as steady:
            for _ in range(timesteps - 1):
                torch.cuda.synchronize(self.device)
                start = time.time()
                repeated = self.repeated_steps
                for i in range(len(inputs)):
                    self._slot0 = i  # each scene keeps its own buffer-size estimates
                    inputs[i] = self.run_inference(inputs[i:i + 1])[0]
                self._slot0 = 0
                torch.cuda.synchronize(self.device)
                timing.append(time.time() - start)
                for i in range(len(inputs)):
                    results[i].append(inputs[i])
                steady.tick(full=self.repeated_steps != repeated)
        self.timing = timing
        if timing:
            log.info("Average runtime: %.05f" % (np.mean(timing) / len(inputs)))
        return results

    def _require_batched_step(self):
        """NotImplementedError naming the model unless it has a batched step -- before anything is launched."""
        check = getattr(self.model, "_check_batched_step", None)
        if check is not None:
            check()
        elif not hasattr(self.model, "step_batched"):
            raise NotImplementedError(f"step_batched: {type(self.model).__name__}")

    @torch.no_grad()
    def run_rollout_batched(self, inputs, timesteps=2):
        """:meth:`run_rollout` with ONE ``model.step_batched`` over all scenes per time step (pipeline key ``valid_batched``)
        instead of one ``run_inference`` per scene: the same inputs, the same ``results[i][t] = [pos, vel, acc, None, box,
        bfeats]`` (scene i's rows of the batched result, sliced by its fluid row splits), ``self.timing`` and the "Average
        runtime" line.  Scene i's frames are the loop's up to the order of float32 additions in the batched kernels.  A model
        without a batched step is a NotImplementedError before anything is launched."""
        self._require_batched_step()
        inputs = [[self._to_device(data["pos"][0]), self._to_device(data["vel"][0]),
                   self._to_device(data["grav"][0]) if data.get("grav") is not None and data["grav"][0] is not None
                   else None, None, self._to_device(data["box"][0]), self._to_device(data["box_normals"][0])]
                  for data in inputs]
        results = [[] for _ in range(len(inputs))]
        self.run_inference(inputs[:1])  # "dummy init": builds the lazily created weights (simulator.py:94)
        timing = []
        for i in range(len(inputs)):
            results[i].append(inputs[i])
        with steady_steps() as steady:
            for _ in range(timesteps - 1):
                torch.cuda.synchronize(self.device)
                start = time.time()
                pos2, vel2, rs = self.model.step_batched(inputs, training=False)
                inputs = [[pos2[rs[i]:rs[i + 1]], vel2[rs[i]:rs[i + 1]]] + list(inputs[i][2:]) for i in range(len(inputs))]
                torch.cuda.synchronize(self.device)
                timing.append(time.time() - start)
                for i in range(len(inputs)):
                    results[i].append(inputs[i])
                steady.tick()
        self.timing = timing
        if timing:
            log.info("Average runtime: %.05f" % (np.mean(timing) / len(inputs)))
        return results

    def load_ckpt(self, ckpt_path):
        """base_pipeline.py:155-187 for inference: read a TensorFlow tensor-bundle checkpoint (``<dir>/ckpt`` prefix, or
        the newest ``ckpt-<n>`` in a directory) into the model; returns the epoch (0 without a checkpoint: the model then
        runs on its initialisers, as the reference does)."""
        from ..utils import tf_checkpoint as tc
        if not ckpt_path:
            log.info("No checkpoint")
            return 0
        prefix, epoch = ckpt_path, 0  # an explicit checkpoint prefix: epoch 0 (base_pipeline.py:171-175)
        if os.path.isdir(ckpt_path):
            import glob
            import re
            idx = sorted(glob.glob(os.path.join(ckpt_path, "*.index")),
                         key=lambda f: [int(x) for x in re.findall(r"\d+", os.path.basename(f))] or [0])
            if not idx:
                log.info("No checkpoint")
                return 0
            prefix = idx[-1][:-len(".index")]
            # the newest checkpoint of a directory (manager.latest_checkpoint): 'ckpt-<n>' was written at the end of epoch
            # (n - 1) * save_ckpt_freq, the run continues with the next one (base_pipeline.py:176-185)
            epoch = tc.checkpoint_epoch(prefix, int(self.cfg.get("save_ckpt_freq", 1) or 1))
        log.info("Loading checkpoint %s", prefix)
        tc.load_into_model(self.model, tc.load_checkpoint(prefix), device=self.device)
        return epoch

    def run_test(self, epoch=None):
        """simulator.py:111-165: roll out every scene of the test split over its full length and write
        ``<out_dir>/visual/<scene>/<epoch>.hdf5`` with the datasets pred / gt / bnd (an HDF5 file utils/draw_sim2d.py reads:
        through h5py when installed, else by the built-in writer).  Returns the list of output paths."""
        from ..datasets import get_rollout, write_results
        cfg = self.cfg
        gen = dict(cfg.get("data_generator") or {})
        test_kw = dict(gen.pop("test", None) or {})
        for k in ("train", "valid"):
            gen.pop(k, None)
        test_data = get_rollout(self.dataset.test, **gen, **test_kw)
        if epoch is None:
            epoch = self.load_ckpt(self.model.cfg.get("ckpt_path"))
        log.info("Started testing")
        results = self.run_rollout(test_data, test_data[0]["pos"].shape[0])
        paths = []
        for i in range(len(results)):
            data = test_data[i]
            pos = np.stack([r[0].cpu().numpy() for r in results[i]])
            out_dir = os.path.join(cfg.out_dir, "visual", "%04d" % i)
            os.makedirs(out_dir, exist_ok=True)
            output = [(pos, {"name": "pred", "type": "PARTICLE"}), (data["pos"], {"name": "gt", "type": "PARTICLE"}),
                      (data["box"][0], {"name": "bnd", "type": "PARTICLE"})]
            path = os.path.join(out_dir, "%04d.hdf5" % epoch)
            write_results(path, self.model.name, output)
            # simulator.py:155-162: write first, THEN drop the scene directory's other result files (a failed write must not
            # cost the previous results)
            for stale in os.listdir(out_dir):
                if stale.endswith((".hdf5", ".npz")) and os.path.join(out_dir, stale) != path:
                    os.remove(os.path.join(out_dir, stale))
            paths.append(path)
        if cfg.get("test_compute_metric", False):  # simulator.py:164-165
            self.run_valid(epoch)
        return paths

    def _data_generator(self, split):
        """``cfg.data_generator`` merged with its ``split`` section (``**cfg.data_generator, **cfg.data_generator.<split>``)."""
        gen = dict(self.cfg.get("data_generator") or {})
        kw = dict(gen.get(split) or {})
        for k in ("train", "valid", "test"):
            gen.pop(k, None)
        return gen, kw

    @torch.no_grad()
    def run_valid(self, epoch=None):
        """simulator.py:167-285: roll out every scene of the validation split (``get_rollout(dataset.valid,
        **data_generator, **data_generator.valid)``), then every ``eval_stride`` frames t >= 1 compare the prediction with
        the target: ``mse_val``, ``chamfer_val``, ``mse_single_val`` (one step from the target's frame t - 1) and, unless the
        split is "train", ``dens_val``, ``max_dens_val``, ``chamfer_val_2``, ``emd``, ``vel_diff_val``, ``vel_diff_val_2``.
        Logs the per-scene means and the overall means (with their sum ``loss``) to ``<logs_dir>/log_valid_<time>.txt``;
        returns the overall dict, also kept as ``self.valid_loss``."""
        from ..datasets import get_rollout
        from ..utils.evaluation_helper import chamfer_distance, compare_dist, distance, merge_dicts
        from ..utils.tools.losses import density_loss, emd_loss, get_window_func
        cfg, model = self.cfg, self.model
        # pipeline key valid_batched (default false): one batched step per rollout step and per-frame metrics over all scenes
        valid_batched = bool(cfg.get("valid_batched", False))
        if valid_batched:
            self._require_batched_step()  # (NotImplementedError for a model without a batched step, before any launch)
        os.makedirs(cfg.logs_dir, exist_ok=True)
        timestamp = datetime.now().strftime("%Y-%m-%d_%H:%M:%S")
        log_file_path = os.path.join(cfg.logs_dir, "log_valid_" + timestamp + ".txt")
        log.info("Logging in file : {}".format(log_file_path))
        handler = logging.FileHandler(log_file_path)
        level = log.level
        if not log.isEnabledFor(logging.INFO):
            log.setLevel(logging.INFO)
        log.addHandler(handler)
        try:
            gen, valid_kw = self._data_generator("valid")
            valid_data = get_rollout(self.dataset.valid, **gen, **valid_kw)
            if epoch is None:
                epoch = self.load_ckpt(model.cfg.get("ckpt_path"))
            log.info("Started validation")
            rollout = self.run_rollout_batched if valid_batched else self.run_rollout
            results = rollout(valid_data, valid_data[0]["pos"].shape[0])
            eval_stride = valid_kw.get("eval_stride", 1)
            dev = lambda a: self._to_device(a)  # noqa: E731
            batched = self.valid_losses_batched(valid_data, results, eval_stride) if valid_batched else None
            losses = []
            for i in range(len(valid_data)):
                data = valid_data[i]
                target_pos, target_vel = data["pos"], data["vel"]
                box = data["box"][0]
                box_d = dev(box)
                loss_seq = []
                for t in range(1, target_pos.shape[0]):
                    pos, vel = results[i][t][:2]
                    if t % eval_stride != 0:
                        continue
                    if batched is not None:  # (evaluated above, frame by frame over all scenes: the same dict, key for key)
                        losses.append(batched[i][t])
                        loss_seq.append(batched[i][t])
                        continue
                    loss = {}
                    if box.shape[0] > 0:
                        pos = torch.clamp(pos, dev(np.min(box, axis=0)), dev(np.max(box, axis=0)))
                    tgt = dev(target_pos[t])
                    loss["mse_val"] = float(np.mean(distance(target_pos[t], pos)))
                    loss["chamfer_val"] = float(np.mean(chamfer_distance(tgt, pos).astype(np.float32)))
                    if cfg.get("split") != "train":
                        # the reference's argument order, kept as it is: dens_val's target densities are taken over
                        # gt_in = pos + box (the PREDICTION's particles) and its prediction's over target + box;
                        # max_dens_val passes the prediction as gt and the target as pred
                        pos_in, tgt_in = torch.cat([pos, box_d]), torch.cat([tgt, box_d])
                        loss["dens_val"] = float(density_loss(tgt, pos, pos_in, tgt_in, win=get_window_func("poly6")).mean())
                        loss["max_dens_val"] = float(density_loss(pos, tgt, pos_in, tgt_in, radius=model.particle_radii[0],
                                                                  win=get_window_func(model.window_dens), use_max=True))
                        loss["chamfer_val_2"] = float(np.mean(chamfer_distance(pos, tgt).astype(np.float32)))
                        loss["emd"] = float(np.mean(emd_loss(tgt.unsqueeze(0), pos.unsqueeze(0)).cpu().numpy().astype(np.float32)))
                        loss["vel_diff_val"] = compare_dist(target_vel[t], vel)
                        loss["vel_diff_val_2"] = compare_dist(vel, target_vel[t])
                    # mse for a single step only: one model step from the target's previous frame
                    pos_sub = self.run_inference([[dev(target_pos[t - 1]), dev(target_vel[t - 1])] + list(results[i][t][2:])])[0][0]
                    loss["mse_single_val"] = float(np.mean(distance(target_pos[t], pos_sub)))
                    losses.append(loss)
                    loss_seq.append(loss)
                loss_m = merge_dicts(loss_seq, lambda x, y: x + y / len(loss_seq))
                desc = "%d -" % i
                for k, v in loss_m.items():
                    desc += " %s: %.05f" % (k, v)
                log.info(desc)
            loss = merge_dicts(losses, lambda x, y: x + y / len(losses))
            sum_loss = 0
            desc = "validation of epoch %d -" % epoch
            for k, v in loss.items():
                desc += " %s: %.05f" % (k, v)
                sum_loss += v
            desc += " > loss: %.05f" % sum_loss
            loss["loss"] = sum_loss
            log.info(desc)
        finally:
            log.removeHandler(handler)
            handler.close()
            log.setLevel(level)
        self.valid_loss = loss
        return loss

    @torch.no_grad()
    def valid_losses_batched(self, valid_data, results, eval_stride=1):
        """The metrics of :meth:`run_valid` with pipeline key ``valid_batched``: every evaluated frame t for ALL scenes that
        have a frame t at once (:func:`valid_frames`).  -> ``losses[i][t]``, the dict the loop builds for scene i's frame t,
        key for key in the loop's order.

        Per frame: the clamp to every scene's box with per-row bounds; ONE dmcf_nn_distance_ragged call for ``chamfer_val``
        and (unless the split is "train") ``chamfer_val_2`` -- the two directions of nn_distance(pos, target); two batched
        density_loss calls for ``dens_val`` / ``max_dens_val`` (the reference's argument orders kept); ONE model.step_batched
        from the targets' frames t - 1 for ``mse_single_val``.  The per-point arrays reach the host in one copy per frame, and
        the per-scene means are np.mean over the same float32 arrays as in the loop: they equal the loop's bit for bit
        wherever the device arrays do.  ``emd`` is ONE emd_loss call with row splits (dmcf_emd_ragged: every scene's cost has
        the bits of the loop's per-scene call), its [scenes] result travelling in the same host copy.  The two
        ``vel_diff_val*`` are ONE ops.hist_pair_ragged call (dmcf_hist_pair_ragged) on the concatenated target and predicted
        velocities: its integer bin counts travel in the same host copy, and evaluation_helper._kl_from_counts -- the last
        lines of compare_dist -- turns them into KL(target || pred) and KL(pred || target), the loop's bits.  A frame whose
        velocities are not float32 [count, 3] on both sides keeps the loop's per-scene host code."""
        from ..utils.evaluation_helper import _kl_pairs, compare_dist, distance
        from ..utils.tools.losses import density_loss, emd_loss, get_window_func
        cfg, model, dev = self.cfg, self.model, self._to_device
        full = cfg.get("split") != "train"
        boxes = [data["box"][0] for data in valid_data]
        boxes_d = [dev(box) for box in boxes]
        # per-scene clamp bounds (the loop's np.min / np.max of the box; a scene without a box is not clamped)
        inf = np.float32(np.inf)
        bounds = np.stack([np.concatenate([np.min(box, axis=0), np.max(box, axis=0)]).astype(np.float32) if box.shape[0] > 0
                           else np.array([-inf] * 3 + [inf] * 3, dtype=np.float32) for box in boxes])
        losses = [dict() for _ in valid_data]
        for t, scenes in valid_frames([data["pos"].shape[0] for data in valid_data], eval_stride):
            counts = [int(results[i][t][0].shape[0]) for i in scenes]
            rs = [0]
            for c in counts:
                rs.append(rs[-1] + c)
            tcounts = [int(valid_data[i]["pos"][t].shape[0]) for i in scenes]
            trs = [0]
            for c in tcounts:
                trs.append(trs[-1] + c)
            n = rs[-1]
            lohi = dev(np.repeat(bounds[scenes], counts, axis=0))
            pos = torch.clamp(torch.cat([results[i][t][0] for i in scenes]), lohi[:, :3], lohi[:, 3:])
            tgt = dev(np.concatenate([valid_data[i]["pos"][t] for i in scenes]))
            d_pos, _, d_tgt, _ = ops.nn_distance_ragged(pos, tgt, rs, trs, want2=full)
            parts = [pos.reshape(-1), torch.sqrt(d_pos)]
            if full:
                # the reference's argument order, kept as it is (see the loop in run_valid)
                in_rs = [0]
                for k, i in enumerate(scenes):
                    in_rs.append(in_rs[-1] + counts[k] + boxes_d[i].shape[0])
                pos_in = torch.cat([x for k, i in enumerate(scenes) for x in (pos[rs[k]:rs[k + 1]], boxes_d[i])])
                tgt_in = torch.cat([x for k, i in enumerate(scenes) for x in (tgt[trs[k]:trs[k + 1]], boxes_d[i])])
                dens = density_loss(tgt, pos, pos_in, tgt_in, win=get_window_func("poly6"), row_splits=rs, in_row_splits=in_rs)
                max_dens = density_loss(pos, tgt, pos_in, tgt_in, radius=model.particle_radii[0],
                                        win=get_window_func(model.window_dens), use_max=True, row_splits=rs, in_row_splits=in_rs)
                parts += [torch.sqrt(d_tgt), dens, max_dens, emd_loss(tgt, pos, true_row_splits=trs, pred_row_splits=rs)]
                # both vel_diff_val: the histograms of target and predicted velocities of all scenes in one call; the int32
                # counts travel as bits in the float32 concatenation.  Anything but float32 [count, 3] on both sides: the
                # loop's host code for this frame
                tvel, pvel = [valid_data[i]["vel"][t] for i in scenes], [results[i][t][1] for i in scenes]
                hist_offsets = None
                if all(isinstance(a, np.ndarray) and a.dtype == np.float32 and isinstance(b, torch.Tensor) and b.is_cuda
                       and b.dtype == torch.float32 and a.shape == tuple(b.shape) == (c, 3) and c > 0
                       for a, b, c in zip(tvel, pvel, counts)):
                    _, hist_counts, hist_offsets = ops.hist_pair_ragged(dev(np.concatenate(tvel)), torch.cat(pvel), rs)
                    parts.append(hist_counts.view(torch.float32))
            # mse for a single step only: one batched model step from the targets' previous frames
            items = [[dev(valid_data[i]["pos"][t - 1]), dev(valid_data[i]["vel"][t - 1])] + list(results[i][t][2:]) for i in scenes]
            pos_sub, _, srs = model.step_batched(items, training=False)
            parts.append(pos_sub.reshape(-1))
            host = torch.cat(parts).cpu().numpy()  # the frame's one host copy of the per-point arrays
            chunks = np.split(host, np.cumsum([int(x.numel()) for x in parts])[:-1])
            pos_h, cham, sub_h = chunks[0].reshape(n, 3), chunks[1], chunks[-1].reshape(srs[-1], 3)
            if full:
                cham2, dens_h, max_dens_h, emd_h = chunks[2:6]
                if hist_offsets is not None:
                    kl_tp, kl_pt = _kl_pairs(chunks[6].view(np.int32), hist_offsets)
            for k, i in enumerate(scenes):
                data = valid_data[i]
                a, b = rs[k], rs[k + 1]
                loss = {}
                loss["mse_val"] = float(np.mean(distance(data["pos"][t], pos_h[a:b])))
                loss["chamfer_val"] = float(np.mean(cham[a:b].astype(np.float32)))
                if full:
                    loss["dens_val"] = float(dens_h[k])
                    loss["max_dens_val"] = float(max_dens_h[k])
                    loss["chamfer_val_2"] = float(np.mean(cham2[trs[k]:trs[k + 1]].astype(np.float32)))
                    loss["emd"] = float(emd_h[k])
                    if hist_offsets is not None:
                        loss["vel_diff_val"], loss["vel_diff_val_2"] = float(kl_tp[k]), float(kl_pt[k])
                    else:
                        vel = results[i][t][1]
                        loss["vel_diff_val"] = compare_dist(data["vel"][t], vel)
                        loss["vel_diff_val_2"] = compare_dist(vel, data["vel"][t])
                loss["mse_single_val"] = float(np.mean(distance(data["pos"][t], sub_h[srs[k]:srs[k + 1]])))
                losses[i][t] = loss
        return losses


    def train_loader(self, schedule):
        """get_dataloader(dataset.train, batch_size, pre_frames, window, **data_generator, **data_generator.train)
        (simulator.py:297-305 and the rebuilds of :438-458)."""
        from ..datasets import get_dataloader
        gen, kw = self._data_generator("train")
        kw.pop("seed", None)
        self._loader_seed = getattr(self, "_loader_seed", -1) + 1
        return get_dataloader(self.dataset.train, batch_size=self.cfg.batch_size, pre_frames=schedule.pre_frames,
                              window=schedule.window, seed=int(self.cfg.get("seed", 0)) + 7919 * self._loader_seed, **gen, **kw)

    def make_optimizer(self):
        """KerasAdam over every built weight of the model (checkpoint order), from ``cfg.optimizer`` and ``grad_clip_norm``."""
        from ..utils import tf_checkpoint as tc
        from ..utils.tools.losses import KerasAdam
        self._variables = tc.model_variables(self.model)
        params = [getattr(mod, attr) for _, mod, attr in self._variables]
        named = {id(p) for p in params}
        params += [p for p in self.model.parameters() if id(p) not in named]  # (weights without a checkpoint name: none today)
        self.optimizer = KerasAdam.from_config(params, self.cfg.optimizer, clip_norm=self.cfg.get("grad_clip_norm", -1))
        return self.optimizer

    def restore_train_state(self, ckpt_path=None):
        """base_pipeline.py:155-187 for training: an explicit ``ckpt_path`` restores the weights, the Adam slots, ``iter`` and
        ``save_counter`` and the run starts at epoch 0; otherwise the newest ``ckpt-<n>`` of ``<logs_dir>/checkpoint`` restores
        the same and the run continues at epoch ``(n - 1) save_ckpt_freq + 1``.  Call after the weights are built;
        builds the optimizer.  Returns the start epoch."""
        from ..utils import tf_checkpoint as tc
        self.manager = tc.CheckpointManager(os.path.join(self.cfg.logs_dir, "checkpoint"), max_to_keep=100)
        self.save_counter, self.object_graph, epoch = 0, None, 0
        prefix = ckpt_path or self.manager.latest_checkpoint
        if prefix:
            weights, slots, opt, graph = tc.read_train_state(prefix)
            tc.load_into_model(self.model, weights, device=self.device)
            self.object_graph = graph
            # tf.train.Checkpoint.restore restores save_counter from any checkpoint, an explicit one included, and the manager
            # numbers its next checkpoint save_counter + 1: a run fine-tuned from a checkpoint with save_counter 51 writes
            # ckpt-52 first
            self.save_counter = int(opt.get("save_counter", 0))
            if not ckpt_path:
                epoch = tc.checkpoint_epoch(prefix, int(self.cfg.get("save_ckpt_freq", 1) or 1))
            log.info("Restored from %s", prefix)
        else:
            log.info("Initializing from scratch.")
        opt_ = self.make_optimizer()
        if prefix:
            opt_.iterations = int(opt.get("iter", 0))
            for k in ("beta_1", "beta_2", "decay"):
                if k in opt:
                    setattr(opt_, k, float(opt[k]))
            for key, mod, attr in self._variables:
                if key in slots and "m" in slots[key] and "v" in slots[key]:
                    opt_.set_slots(getattr(mod, attr), slots[key]["m"], slots[key]["v"])
        return epoch

    def save_ckpt(self, epoch):
        """CheckpointManager.save (base_pipeline.py:189-191): ``ckpt-<save_counter + 1>``."""
        self.save_counter += 1
        path = self.manager.save(self.model, self.optimizer, self.save_counter, self.object_graph)
        log.info("Saved checkpoint at: %s", path)
        return path

    def _sample_tensors(self, data, bi):
        dev = self._to_device
        grav = data["grav"][bi]
        return dict(pos=data["pos"][bi], grav0=dev(grav[0]) if grav[0] is not None else None, box0=dev(data["box"][bi][0]),
                    boxn0=dev(data["box_normals"][bi][0]))

    def warm_up(self, data, max_err=None, max_dens_err=None):
        """simulator.py:325-368 on the inference path (no gradients): per sample up to ``pre`` model steps from frame 0, with
        the ``max_err`` / ``max_dens_err`` early exits.  Restated as written: the state after p + 1 steps is compared with
        frame p, and a warm-up that runs all k steps hands on pre = k - 1, the last loop index, with the state of frame k
        (DESIGN.md section 4.9).  -> (in_pos, in_vel, pre) lists."""
        from ..utils.tools.losses import density_loss, get_window_func
        model = self.model
        in_pos, in_vel, pres = [], [], []
        with torch.no_grad():
            for bi in range(len(data["pos"])):
                s = self._sample_tensors(data, bi)
                pr_pos, pr_vel = self._to_device(data["pos"][bi][0]), self._to_device(data["vel"][bi][0])
                p = 0
                prev_err, prev_dens_err = 0.0, 0.0
                for p in range(int(data["pre"][bi])):
                    pos, vel = model([pr_pos, pr_vel, s["grav0"], None, s["box0"], s["boxn0"]], training=False)
                    frame = self._to_device(s["pos"][p])
                    if max_err is not None:
                        err = float(torch.max(torch.sum(torch.abs(pos - frame), dim=-1)))
                        if p > 0 and err > prev_err and err > max_err:
                            break
                        prev_err = err
                    if max_dens_err is not None:
                        # the reference's argument order: the prediction as gt, the frame as pred
                        err = float(density_loss(pos, frame, torch.cat([pos, s["box0"]]), torch.cat([frame, s["box0"]]),
                                                 radius=model.particle_radii[0], win=get_window_func(model.window_dens),
                                                 use_max=True))
                        if p > 0 and err > prev_dens_err and err > max_dens_err:
                            break
                        prev_dens_err = err
                    pr_pos, pr_vel = pos, vel
                pres.append(p)
                in_pos.append(pr_pos)
                in_vel.append(pr_vel)
        return in_pos, in_vel, pres

    def warm_up_batched(self, data, max_err=None, max_dens_err=None):
        """:meth:`warm_up` with ONE ``model.step_batched`` per iteration over the samples that are still warming up (pipeline key
        ``warm_up_batched``): at iteration p those with ``pre > p`` that have not left.  The ``max_err`` errors of all items
        come from one chain of torch ops on the concatenated rows, the ``max_dens_err`` errors from one batched density_loss
        (two dmcf_frs_window_sum_batched launches with the per-item maxima), and both are read back in one host copy per
        iteration.  The exits are decided per sample on the host (:class:`WarmUpExits`) as the loop decides them; a sample that
        left or finished is not in the next iteration's batch.  -> (in_pos, in_vel, pre) lists, the contract of warm_up; item
        b's state is the loop's up to the order of float32 additions in the batched kernels."""
        from ..utils.tools.losses import density_loss, get_window_func
        model = self.model
        self._require_batched_step()  # (NotImplementedError for a model without a batched step, before any launch)
        n = len(data["pos"])
        exits = WarmUpExits(data["pre"], max_err, max_dens_err)
        with torch.no_grad():
            samples = [self._sample_tensors(data, bi) for bi in range(n)]
            pr_pos = [self._to_device(data["pos"][bi][0]) for bi in range(n)]
            pr_vel = [self._to_device(data["vel"][bi][0]) for bi in range(n)]
            for p in range(max(exits.pre, default=0)):
                active = exits.active(p)
                if not active:
                    break
                items = [[pr_pos[bi], pr_vel[bi], samples[bi]["grav0"], None, samples[bi]["box0"], samples[bi]["boxn0"]]
                         for bi in active]
                pos2, vel2, rs = model.step_batched(items, training=False)
                errs = []
                if max_err is not None or max_dens_err is not None:
                    frames = [self._to_device(samples[bi]["pos"][p]) for bi in active]
                    frame = torch.cat(frames)
                if max_err is not None:
                    counts = torch.tensor([rs[k + 1] - rs[k] for k in range(len(active))], device=pos2.device)
                    item = torch.repeat_interleave(torch.arange(len(active), device=pos2.device), counts, output_size=rs[-1])
                    row = torch.sum(torch.abs(pos2 - frame), dim=-1)
                    errs.append(torch.zeros(len(active), dtype=row.dtype, device=row.device).scatter_reduce(
                        0, item, row, "amax", include_self=False))
                if max_dens_err is not None:
                    # the reference's argument order: the prediction as gt, the frame as pred; per item over [pos_b, box0_b]
                    # and [frame_b, box0_b]
                    boxes = [samples[bi]["box0"] for bi in active]
                    in_rs = [0]
                    for k, box in enumerate(boxes):
                        in_rs.append(in_rs[-1] + rs[k + 1] - rs[k] + box.shape[0])
                    pos_in = torch.cat([t for k, box in enumerate(boxes) for t in (pos2[rs[k]:rs[k + 1]], box)])
                    frame_in = torch.cat([t for f, box in zip(frames, boxes) for t in (f, box)])
                    errs.append(density_loss(pos2, frame, pos_in, frame_in, radius=model.particle_radii[0],
                                             win=get_window_func(model.window_dens), use_max=True, row_splits=list(rs),
                                             in_row_splits=in_rs))
                host = torch.stack(errs).tolist() if errs else []  # the iteration's one host copy
                err = host[0] if max_err is not None else None
                dens_err = host[-1] if max_dens_err is not None else None
                for k, bi in enumerate(active):
                    if exits.accept(p, bi, None if err is None else err[k], None if dens_err is None else dens_err[k]):
                        pr_pos[bi], pr_vel[bi] = pos2[rs[k]:rs[k + 1]], vel2[rs[k]:rs[k + 1]]
        return pr_pos, pr_vel, exits.pres()

    def window_loss(self, data, time_w, in_pos, in_vel, pres, it=0):
        """simulator.py:370-403 on the recording path: per sample, ``len(time_w)`` model steps from the warmed-up state with
        gradients through all of them; the step-t losses against target frame t + pre + 1 (previous frame t + pre), weighted
        by time_w[t]; summed over the samples and divided by sum(time_w) * batch; plus ``w_decay`` sum w^2.  -> the loss
        vector (one entry per model.loss_keys())."""
        model = self.model
        if it > 1:
            # simulator.py:386-391 calls model(inputs, vel, training=True): Keras rejects the second positional argument next
            # to training=..., so the reference cannot run it either (every shipped config has iterations: [0])
            raise NotImplementedError("iterations > 1 (the reference's inner iteration loop cannot run)")
        model.requires_grad_(True)
        tw = torch.as_tensor(np.asarray(time_w, dtype=np.float32), device=self.device)
        set_rows = []  # (the weighted rows of the train_set_losses columns, when the key is set)
        if self.cfg.get("train_batched", False):  # pipeline key train_batched (default false): one batched step per window step
            rows = self._window_rows_batched(data, tw, in_pos, in_vel, pres, set_rows)
        else:
            rows = self._window_rows(data, tw, in_pos, in_vel, pres)
        loss_sum = torch.stack(rows).sum(0) / (tw.sum() * len(data["pos"]))
        if set_rows:
            # the columns of train_set_losses, summed apart from the model's: those keep the bits they have without the key
            loss_sum = torch.cat([loss_sum, torch.stack(set_rows).sum(0) / (tw.sum() * len(data["pos"]))])
        w_decay = self.cfg.get("w_decay", 0) or 0
        if w_decay > 0:
            # a scalar added to every entry of the loss vector (simulator.py:407-410: w_decay * reduce_sum of the per-weight sums)
            loss_sum = loss_sum + w_decay * torch.stack([torch.sum(w ** 2) for w in self.optimizer.params]).sum()
        return loss_sum

    def _window_rows(self, data, tw, in_pos, in_vel, pres):
        """The weighted per-step losses of window_loss, sample after sample."""
        from ..utils.evaluation_helper import merge_dicts
        model = self.model
        rows = []
        for bi in range(len(data["pos"])):
            s = self._sample_tensors(data, bi)
            pos, vel, pre = in_pos[bi], in_vel[bi], int(pres[bi])
            for t in range(tw.shape[0]):
                inputs = [pos, vel, s["grav0"], None, s["box0"], s["boxn0"]]
                pos, vel = model(inputs, training=True)
                target = s["pos"]
                ls = [model.loss([pos, vel], [inputs, self._to_device(target[t + pre + 1]), self._to_device(target[t + pre]), pre])]
                ls = merge_dicts(ls, lambda x, y: x + y / len(ls))
                rows.append(torch.stack([torch.as_tensor(v, device=self.device).reshape(()) for v in ls.values()]) * tw[t])
        return rows

    def _window_rows_batched(self, data, tw, in_pos, in_vel, pres, set_rows=None):
        """The weighted per-step losses of window_loss with pipeline key ``train_batched``: each of the len(time_w) steps is ONE
        model.step_batched over all samples, and every sample's loss is formed by model.loss on that sample's rows of pos2,
        pos_correction and num_fluid_neighbors.  The same terms as the per-sample loop, sample-major order of the rows aside
        (they are summed).  With ``train_set_losses`` the sample's weighted Chamfer / EMD columns of the step are appended to
        ``set_rows``, row for row (:meth:`_set_loss_columns`: one ragged call per name and step)."""
        from ..utils.evaluation_helper import merge_dicts
        model = self.model
        samples = [self._sample_tensors(data, bi) for bi in range(len(data["pos"]))]
        pos, vel = list(in_pos), list(in_vel)
        rows = []
        for t in range(tw.shape[0]):
            items = [[pos[bi], vel[bi], s["grav0"], None, s["box0"], s["boxn0"]] for bi, s in enumerate(samples)]
            pos2, vel2, rs = model.step_batched(items, training=True)
            correction, neighbors = model.pos_correction, model.num_fluid_neighbors
            extra = None
            if self.set_losses and set_rows is not None:
                extra = self._set_loss_columns(pos2, rs, [self._to_device(s["pos"][t + int(pres[bi]) + 1])
                                                          for bi, s in enumerate(samples)])
            try:
                for bi, s in enumerate(samples):
                    a, b, pre = rs[bi], rs[bi + 1], int(pres[bi])
                    pos[bi], vel[bi] = pos2[a:b], vel2[a:b]
                    model.pos_correction, model.num_fluid_neighbors = correction[a:b], neighbors[a:b]
                    target = s["pos"]
                    ls = [model.loss([pos[bi], vel[bi]], [items[bi], self._to_device(target[t + pre + 1]),
                                                          self._to_device(target[t + pre]), pre])]
                    ls = merge_dicts(ls, lambda x, y: x + y / len(ls))
                    rows.append(torch.stack([torch.as_tensor(v, device=self.device).reshape(()) for v in ls.values()]) * tw[t])
                    if extra is not None:
                        set_rows.append(extra[bi] * tw[t])
            finally:
                model.pos_correction, model.num_fluid_neighbors = correction, neighbors
        return rows

    def train_step(self, data, time_w, it=0, max_err=None, max_dens_err=None):
        """The reference's ``train(data, time_w, it, max_err, max_dens_err)`` (simulator.py:318-414): warm-up, the recorded
        window, backward, KerasAdam.  ``data``: one batch of get_dataloader.  The model's weights must be built (run_train
        makes one inference call first): the optimizer takes the weights that exist when it is made.  -> (loss vector as numpy, pre list).  Times the
        phases into ``self.train_timing`` (warm_up, forward, backward, optimizer; seconds, device-synchronised)."""
        if self.optimizer is None:
            self.make_optimizer()
        if getattr(self.model, "shard", None) is not None:
            raise NotImplementedError("training in the sharded step")
        sync = lambda: torch.cuda.synchronize(self.device)  # noqa: E731
        t0 = time.perf_counter()
        # pipeline key warm_up_batched (default false): one batched step per warm-up iteration instead of the per-sample loop
        warm_up = self.warm_up_batched if self.cfg.get("warm_up_batched", False) else self.warm_up
        in_pos, in_vel, pres = warm_up(data, max_err, max_dens_err)
        sync()
        t1 = time.perf_counter()
        self.optimizer.zero_grad()
        loss_sum = self.window_loss(data, time_w, in_pos, in_vel, pres, it)
        sync()
        t2 = time.perf_counter()
        loss_sum.sum().backward()  # (tape.gradient of a vector: the gradient of its sum)
        sync()
        t3 = time.perf_counter()
        self.optimizer.step()
        sync()
        t4 = time.perf_counter()
        self.train_timing = dict(warm_up=t1 - t0, forward=t2 - t1, backward=t3 - t2, optimizer=t4 - t3)
        return loss_sum.detach().cpu().numpy(), pres

    def run_train(self):
        """simulator.py:287-518: the training loop.  Logs ``training - <key>: ... > loss: ...`` per iteration to
        ``<logs_dir>/log_train_<time>.txt`` (no TensorBoard); checkpoint every ``save_ckpt_freq`` epochs, run_valid and
        run_test after every epoch.  Returns the last iteration's loss dict."""
        cfg, model = self.cfg, self.model
        os.makedirs(cfg.logs_dir, exist_ok=True)
        timestamp = datetime.now().strftime("%Y-%m-%d_%H:%M:%S")
        handler = logging.FileHandler(os.path.join(cfg.logs_dir, "log_train_" + timestamp + ".txt"))
        level = log.level
        if not log.isEnabledFor(logging.INFO):
            log.setLevel(logging.INFO)
        log.addHandler(handler)
        try:
            # pipeline key train_lattice_form (default false): recording layers between two grid_pos lattices keep the stencil
            # form and its own backward (ContinuousConv(record_lattice_form=True))
            if hasattr(model, "record_lattice_form"):
                model.record_lattice_form(bool(cfg.get("train_lattice_form", False)))
            # pipeline key train_scatter_form (default false): recording particles -> lattice layers with 4 or 8 output channels
            # take the input-stationary backward on the transposed list (ContinuousConv(record_scatter_form=True))
            if hasattr(model, "record_scatter_form"):
                model.record_scatter_form(bool(cfg.get("train_scatter_form", False)))
            schedule = TrainSchedule(cfg)
            loader = self.train_loader(schedule)
            first = next(loader)
            # build the lazily created weights before the optimizer takes them ("dummy init", simulator.py:94)
            with torch.no_grad():
                s = self._sample_tensors(first, 0)
                model([self._to_device(first["pos"][0][0]), self._to_device(first["vel"][0][0]), s["grav0"], None, s["box0"],
                       s["boxn0"]], training=False)
            start_ep = self.restore_train_state(model.cfg.get("ckpt_path"))
            pending = [first]
            log.info("Started training")
            loss = {}
            for epoch in range(start_ep, cfg.max_epoch + 1):
                log.info(f"=== EPOCH {epoch:d}/{cfg.max_epoch:d} ===")
                for i in range(cfg.iter):
                    step = epoch * cfg.iter + i
                    if schedule.advance(step):
                        loader, pending = self.train_loader(schedule), []
                    t0 = time.perf_counter()
                    data = pending.pop() if pending else next(loader)
                    time_w = schedule.time_weights([d.shape[0] for d in data["pos"]], data["pre"], step)
                    t_data = time.perf_counter() - t0
                    loss_l, pre = self.train_step(data, time_w, schedule.iterations, cfg.get("max_err", None),
                                                  cfg.get("max_dens_err", None))
                    self.train_timing["data"] = t_data
                    loss = {}
                    desc = "training -"
                    for k, v in zip(self.loss_keys(), loss_l):
                        desc += " %s: %.05f" % (k, v)
                        loss[k] = float(v)
                    loss["loss"] = float(np.sum(loss_l))
                    desc += " > loss: %.05f" % loss["loss"]
                    loss["timesteps"] = float(min(np.sum(time_w), np.ceil(np.sum(time_w))))
                    loss["warmup"] = float(np.mean(data["pre"]))
                    loss["warmup_diff"] = float(np.mean(np.asarray(data["pre"]) - np.asarray(pre)))
                    log.info(desc)
                if epoch % cfg.save_ckpt_freq == 0:
                    self.save_ckpt(epoch)
                self.run_valid(epoch)
                self.run_test(epoch)
        finally:
            log.removeHandler(handler)
            handler.close()
            log.setLevel(level)
        self.train_loss = loss
        return loss


class TrainSchedule:
    """The schedules of the training loop, simulator.py:430-480: ``window_it`` / ``warm_up_it`` / ``it_idx`` advance while
    ``step`` has reached the next entry of ``window_bnds`` / ``warm_up_bnds`` / ``its_bnds`` (each bounded by the shorter of
    the two lists); a change of the window or the warm-up rebuilds the loader.  ``time_weights`` is the ``time_w`` blend."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.window_it = self.warm_up_it = self.it_idx = 0

    def advance(self, step):
        """-> True when the loader must be rebuilt for this step (the window or the warm-up changed)."""
        cfg, rebuild = self.cfg, False
        while self.window_it < min(len(cfg.windows), len(cfg.window_bnds)) and step >= cfg.window_bnds[self.window_it]:
            self.window_it += 1
            rebuild = True
        while self.warm_up_it < min(len(cfg.max_warm_up), len(cfg.warm_up_bnds)) and step >= cfg.warm_up_bnds[self.warm_up_it]:
            self.warm_up_it += 1
            rebuild = True
        while self.it_idx < min(len(cfg.iterations), len(cfg.its_bnds)) and step >= cfg.its_bnds[self.it_idx]:
            self.it_idx += 1
        return rebuild

    @property
    def window(self):
        return self.cfg.windows[self.window_it]

    @property
    def pre_frames(self):
        return self.cfg.max_warm_up[self.warm_up_it]

    @property
    def iterations(self):
        return self.cfg.iterations[self.it_idx]

    def time_weights(self, lengths, pres, step):
        """simulator.py:466-478: ones over min(T_b - 1 - pre_b) frames; while a new window blends in (``time_blend`` steps
        after its bound) its last ``windows[k] - windows[k-1]`` weights ramp from ``a`` down by 1 / diff, clipped to [0, 1]."""
        cfg = self.cfg
        time_w = np.ones(int(np.min([t - 1 - p for t, p in zip(lengths, pres)])), dtype=np.float32)
        if self.window_it > 0:
            a = (step - cfg.window_bnds[self.window_it - 1] + 1) / cfg.time_blend
            if a < 1.0 and len(time_w) >= cfg.windows[self.window_it]:
                diff = cfg.windows[self.window_it] - cfg.windows[self.window_it - 1]
                time_w[-diff:] = np.clip(a - np.arange(diff) / diff, 0.0, 1.0)
        return time_w

