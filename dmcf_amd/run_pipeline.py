"""The reference's ``run_pipeline.py`` on the MI355X path: YAML config -> model -> checkpoint -> ``get_rollout`` ->
``Simulator.run_rollout`` (run_pipeline.py:80-154, pipelines/simulator.py:111-285).

    python -m dmcf_amd.run_pipeline -c configs/Liquid3d.yml --split test --dataset_path <dir with *.msgpack.zst> \\
        --ckpt_path checkpoints/Liquid3d/ckpt --output_dir output [--model.timestep 0.02 ...]

Same flags as the reference; ``--section.key value`` overrides go through Config.merge_cfg_file.  ``--split test`` writes
the rollouts (``Simulator.run_test``); ``--split valid`` rolls out the validation split and computes its metrics
(``Simulator.run_valid``: MSE, Chamfer, density, EMD, velocity histograms); ``--split train`` (the default, as in the
reference) runs the training loop (``Simulator.run_train``: scenes from ``<dataset_path>/train``, checkpoints with the Adam
state in ``<logs_dir>/checkpoint``, resumed from the newest one there unless ``--ckpt_path`` is given; ``--restart`` clears
the run's logs and outputs first).  A config without ``dataset_path`` and with ``dataset.type: column`` or ``free_fall`` (the
reference's configs/column/*.yml) has the scenes of the splits it needs GENERATED from the config's ``train`` / ``valid`` /
``test`` sections (datasets/column_gen.py: a HIP 1-D SPH solver; datasets/free_fall_gen.py) and cached under ``cache/``
(``dataset.cache_dir``); ``--regen`` discards the cached scenes.  ``type: tank``, or no type, raises NotImplementedError as the
reference does.
"""
import argparse
import random
import sys

import numpy as np


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Run a network over the test split (run_pipeline.py)")
    parser.add_argument("-c", "--cfg_file", help="path to the config file", required=True)
    parser.add_argument("--dataset_path", help="path to the dataset")
    parser.add_argument("--ckpt_path", help="path to the checkpoint")
    parser.add_argument("--device", help="device to run the pipeline", default="gpu")
    parser.add_argument("--split", help="train, valid or test", default="train")
    parser.add_argument("--regen", default=False, action="store_true")
    parser.add_argument("--restart", default=False, action="store_true")
    parser.add_argument("--main_log_dir", help="the dir to save logs and models")
    parser.add_argument("--output_dir", help="the dir to save outputs")
    args, unknown = parser.parse_known_args(argv)
    extra = argparse.ArgumentParser(description="Extra arguments")  # run_pipeline.py:46-52
    for arg in unknown:
        if arg.startswith(("-", "--")):
            extra.add_argument(arg)
    return args, {k: v for k, v in vars(extra.parse_args(unknown)).items()}


def build(args, extra, data=None):
    """-> the Simulator pipeline of run_pipeline.py:104-121 (``data``: scenes already in memory instead of a dataset_path)."""
    from . import models, pipelines
    from .datasets import DatasetGroup
    from .utils.config import Config
    cfg = Config.load_from_file(args.cfg_file)
    if args.device in ("gpu", None):
        args.device = "cuda"
    Pipeline = getattr(pipelines, cfg.pipeline.name)
    Model = getattr(models, cfg.model.name)
    cfg_dataset, cfg_pipeline, cfg_model = Config.merge_cfg_file(cfg, args, extra)
    dataset = DatasetGroup(**cfg_dataset, split=args.split, regen=args.regen, data=data)
    model = Model(**cfg_model)
    if args.restart:
        cfg_pipeline["restart"] = True
    return Pipeline(model, dataset, **cfg_pipeline)


def main(argv=None, data=None):
    random.seed(42)
    np.random.seed(42)
    args, extra = parse_args(argv)
    if args.split not in ("train", "test", "valid"):
        raise NotImplementedError(f"--split {args.split}: train, valid or test")
    pipeline = build(args, extra, data)
    if args.split == "train":  # run_pipeline.py:147-148
        return pipeline.run_train()
    if args.split == "valid":  # run_pipeline.py:151-152
        return pipeline.run_valid()
    return pipeline.run_test()


if __name__ == "__main__":
    res = main(sys.argv[1:])
    print("\n".join(res) if isinstance(res, list) else "\n".join("%s: %.05f" % kv for kv in res.items()))
