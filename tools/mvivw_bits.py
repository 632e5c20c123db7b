#!/usr/bin/env python3
"""The output bytes of `Engine.mvivw` and `Engine.mvivw_ld` as digests, for comparing two builds of the library on one
device: a change that claims to leave the arithmetic alone must print the same listing as its parent.

One line per case: the SHA-256 over the bytes of theta, se, stats and status, and the SHA-256 over the bytes of the inputs
(which shows that two runs saw the same data).  The cases are the batches of the GPU tests at the smallest sizes on both
sides of every edge of the kernels:
  mvivw     shape_batch(m, k, 0.5) of tests/test_gpu_mvivw.py: (2,1), (257,1), (257,43), (257,44), (257,87), (257,88),
            (128,127), (513,127) -- both sides of each tile class (44 and 88 columns of Z) and of the 256-row chunk --
            and (257,44) at the models 0, 1 and 2; statuses 0 to 3
  mvivw_ld  ld_shape_batch(m, k) of tests/test_gpu_mvivw_ld.py: (65,2), (129,64), (128,127), (257,127), (513,1) -- one
            and several panels and chunks -- and (129,64) at ridge 0.1; statuses 0 to 4
The digests depend on the compiler and the device as well as on the source: compare listings taken together, and keep
none as a fixture.

Usage: python tools/mvivw_bits.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAIN = [(2, 1, 0), (257, 1, 0), (257, 43, 0), (257, 44, 0), (257, 44, 1), (257, 44, 2), (257, 87, 0), (257, 88, 0), (128, 127, 0),
         (513, 127, 0)]
LD = [(65, 2, 0.0), (129, 64, 0.0), (129, 64, 0.1), (128, 127, 0.0), (257, 127, 0.0), (513, 1, 0.0)]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    from cigwas_amd.skeleton import Engine
    from test_gpu_mvivw import call_of, shape_batch
    from test_gpu_mvivw_ld import ld_shape_batch

    eng = Engine(0)
    for m, k, model in PLAIN:
        beta, w, lists, _ = shape_batch(m, k, 0.5)
        call = call_of(lists)
        theta, se, stats, status, _ = eng.mvivw(beta, w, **call, model=model)
        print(f"mvivw m={m} k={k} model={model} status={''.join(map(str, status.tolist()))} "
              f"out={digest((theta, se, stats, status))} in={digest((beta, w, *call.values()))}", flush=True)
    for m, k, ridge in LD:
        beta, w, ld, lists = ld_shape_batch(m, k)
        call = call_of(lists)
        theta, se, stats, status, _ = eng.mvivw_ld(beta, w, ld, **call, ridge=ridge)
        print(f"mvivw_ld m={m} k={k} ridge={ridge} status={''.join(map(str, status.tolist()))} "
              f"out={digest((theta, se, stats, status))} in={digest((beta, w, ld, *call.values()))}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
