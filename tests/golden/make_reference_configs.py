"""Generates tests/golden/reference_configs/: the values of the reference's yaml files that tests/test_shim.py composes and
instantiates (configs/config.yaml, the groups its conv3d experiment selects, and every model yaml), so that those tests
run from this tree alone.

    python tests/golden/make_reference_configs.py <reference checkout>/configs

Each file is loaded and dumped again (keys in their original order): data only, no comments of the reference.
"""
import os
import sys

import yaml

FILES = ["config.yaml", "callbacks/default.yaml", "datamodule/netcdf_datamodule.yaml", "experiment/conv3d.yaml",
         "hydra/default.yaml", "logger/csv.yaml", "trainer/default.yaml", "model/conv3d.yaml", "model/conv3d_nwp.yaml",
         "model/conv3d_sat_nwp.yaml", "model/perceiver.yaml", "model/perceiver_conv3d_sat_nwp.yaml",
         "model/perceiver_sat_nwp.yaml"]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_configs")


def main(src):
    for name in FILES:
        with open(os.path.join(src, name)) as f:
            data = yaml.safe_load(f)
        dst = os.path.join(OUT, name)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "w") as f:
            yaml.safe_dump(data, f, sort_keys=False, default_flow_style=False)


if __name__ == "__main__":
    main(sys.argv[1])
