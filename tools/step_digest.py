#!/usr/bin/env python3
"""Bit digest of one native training step per named case: sha256 over the flat fp32 gradient, and the four losses as hex floats.

A change to the step's host code that must not move a launch or an argument (csrc/vae_step.hip) is checked by running this with the
parent's library and with the head's and comparing the lines: one fresh process per library, chosen with PM_LIB_PATH.

    [PM_LIB_PATH=<other build>] python tools/step_digest.py [case ...]            # no case: all of CASES

The step is `tests/util.py hip_fullsize_step` in deterministic mode with lr = 0: default weights under seed 0, eps of seed 99, batch seed
1234, message dropout 0.1.  A tool, not a test: a digest in the suite would have every legitimate numerics change re-record it.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SPARSE = dict(B=24, nb=2, d=256, L=3, p=0.25, dense=False, msg_p=0.1, seed=1234)
CASES = {
    "d256_sparse_b24_l3": SPARSE,
    "d512_dense_b8_l2": dict(B=8, nb=2, d=512, L=2, p=1.0, dense=True, msg_p=0.1, seed=1234),
    "d256_sparse_b24_l3_fix_structure": dict(SPARSE, fix_structure=True),
    "d256_sparse_b24_l3_dropout": dict(SPARSE, dropout=0.1),
    "d256_sparse_b24_l3_keep_logits_off": dict(SPARSE, keep_logits=False),
}


def main():
    names = sys.argv[1:] or list(CASES)
    unknown = [n for n in names if n not in CASES]
    if unknown:
        sys.exit(f"unknown case(s) {unknown}; known: {list(CASES)}")
    import torch
    from polyphemus_amd import _lib
    from util import hip_fullsize_step
    print(f"# library {os.path.relpath(_lib.LIB_PATH, ROOT)}: {_lib.lib().pm_build_info().decode()}")
    for name in names:
        with _lib.deterministic(True):
            run = hip_fullsize_step(CASES[name], lr=0.0)
        flat = torch.cat([run["grads"][n].reshape(-1) for n in run["names"]]).contiguous()
        assert flat.dtype == torch.float32
        digest = hashlib.sha256(flat.numpy().tobytes()).hexdigest()
        losses = " ".join(f"{k}={float(run['losses'][k]).hex()}" for k in ("pitch", "dur", "structure", "kld"))
        print(f"{name} n={flat.numel()} grad={digest} {losses}", flush=True)


if __name__ == "__main__":
    main()
