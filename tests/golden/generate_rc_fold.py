"""Records tests/golden/rc_fold_base.npz: the final state, log-density and counters of every case of
tests/test_gpu_rc_fold.py, run on a build WITHOUT the folded rough-carpet kernels (the bits the folded kernels must
reproduce).  Needs a GPU; PTRWM_LIB selects the library to record from.

    PTRWM_LIB=<library of the earlier build> python tests/golden/generate_rc_fold.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "rwm-pt-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ptrwm_hip as E  # noqa: E402
import test_gpu_rc_fold as T  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = {}
    for name in T.CASES:
        thread = T.run_case(name, dev, E.FORM_THREAD)
        quad = T.run_case(name, dev, E.FORM_QUAD)
        for k, v in thread.items():
            if k == "launch":
                continue
            assert v.tobytes() == quad[k].tobytes(), (name, k)  # the two forms agree on the recorded build too
            out[f"{name}/{k}"] = v
    np.savez_compressed(os.path.join(HERE, "rc_fold_base.npz"), **out)
    print(f"recorded {len(T.CASES)} cases from {E.LIB_PATH}")


if __name__ == "__main__":
    main()
