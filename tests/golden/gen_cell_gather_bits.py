#!/usr/bin/env python
"""Generates tests/golden/cell_gather_bits.json: case -> output -> SHA-256 of the raw bytes of what voxel_sample, the legacy
trilinear_devoxelize pair, image_sample and tet_centroid_sample return and of every gradient they give, at the cases of
tests/cell_gather_cases.py.  Run ONCE, on the GPU, with the library built from the commit BEFORE the three operators came to share
cell_gather.hpp:

    DEFTET_HIP_LIB=<libdeftet_hip.so built from that commit> python tests/golden/gen_cell_gather_bits.py

tests/test_cell_gather_bits_gpu.py then holds the current library to these digests: the order of every sum is a contract
(DESIGN.md §6i), and the fp64 bounds of the operators' own tests would not notice a changed one.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "cell_gather_bits.json")


def main():
    if not os.environ.get("DEFTET_HIP_LIB"):
        sys.exit("set DEFTET_HIP_LIB to a library built from the commit before cell_gather.hpp")
    sys.path.insert(0, ROOT)
    import torch
    from tests import cell_gather_cases
    if not torch.cuda.is_available():
        sys.exit("gen_cell_gather_bits: needs the GPU")
    out = cell_gather_cases.digests(torch.device("cuda:0"))
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases, %d digests" % (len(out), sum(len(v) for v in out.values())))


if __name__ == "__main__":
    main()
