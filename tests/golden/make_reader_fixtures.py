"""Generates the fixtures of the config and checkpoint reader tests (tests/test_models_cpu.py) from data files of the reference
(tum-pbs/DMCF): ``python tests/golden/make_reader_fixtures.py <reference checkout>``.  The tests only read the committed outputs.

  reference_configs.json  the ``model`` section of configs/<name>.yml for every configuration tools/configs.py restates,
                          as yaml.safe_load reads it (name -> dict)
  liquid3d_ckpt.npz       checkpoints/Liquid3d/ckpt as two uint8 arrays: ``index`` = ckpt.index byte for byte, ``data`` =
                          ckpt.data-00000-of-00001 byte for byte except the Adam slot variables (``.OPTIMIZER_SLOT``, two thirds
                          of the blob), which are zeroed -- tf_checkpoint.load_checkpoint skips them by default
"""
import json
import os
import sys

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dmcf_amd.utils import tf_checkpoint as tc  # noqa: E402
from tools import configs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    REF = sys.argv[1]
    sections = {}
    for name in sorted(configs.BY_NAME):
        with open(os.path.join(REF, "configs", name + ".yml")) as f:
            sections[name] = yaml.safe_load(f)["model"]
    with open(os.path.join(OUT, "reference_configs.json"), "w") as f:
        json.dump(sections, f, indent=1, sort_keys=True)
        f.write("\n")
    prefix = os.path.join(REF, "checkpoints/Liquid3d/ckpt")
    index = open(prefix + ".index", "rb").read()
    data = bytearray(open(prefix + ".data-00000-of-00001", "rb").read())
    zeroed = 0
    for key, e in tc.read_index(prefix + ".index").items():
        if ".OPTIMIZER_SLOT" in key:
            data[e["offset"]:e["offset"] + e["size"]] = bytes(e["size"])
            zeroed += e["size"]
    np.savez_compressed(os.path.join(OUT, "liquid3d_ckpt.npz"), index=np.frombuffer(index, np.uint8),
                        data=np.frombuffer(bytes(data), np.uint8))
    print(sorted(sections), f"checkpoint: {len(data)} data bytes, {zeroed} of them Adam slots (zeroed)")
