"""The child process of tests/test_gpu_xcd_order.py: every case of xcd_order_checks in THIS process, written out as an .npz.

    python tests/xcd_order_child.py <small|large> <out.npz>

The block order in force is whatever the library finds when this process renders its first frame (csrc/frames.cpp: frame_params reads RRT_XCD_CHUNK once per
process), which is why the cases run in a fresh process: the parent puts the chunk into the child's environment.  This script neither sets nor reads anything
of the environment.  Not a test module: pytest does not collect it.
"""
import sys

import numpy as np


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    import xcd_order_checks as X                           # (by bare name: the script's directory leads sys.path; conftest puts the repository root behind it)
    if argv[1] not in X.COLLECTORS:
        print(f"unknown collector {argv[1]!r}: want one of {sorted(X.COLLECTORS)}", file=sys.stderr)
        return 2
    import torch
    out = X.COLLECTORS[argv[1]](X.package(), torch)
    with open(argv[2], "wb") as f:
        np.savez(f, **out)
    print(f"{len(out)} arrays written", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
