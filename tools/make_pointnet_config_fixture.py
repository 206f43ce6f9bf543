"""Write tests/golden/reference_pointnet_config.json: the ``model`` section of the reference's configs/other/pointnet.yml,
the fixture tools/configs.POINTNET2D is checked against (tests/test_pointnet_abi.py).

  python tools/make_pointnet_config_fixture.py <reference tree>"""
import json
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    with open(os.path.join(sys.argv[1], "configs", "other", "pointnet.yml")) as f:
        model = yaml.safe_load(f)["model"]
    out = os.path.join(ROOT, "tests", "golden", "reference_pointnet_config.json")
    with open(out, "w") as f:
        json.dump({"other/pointnet": model}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
