"""Generates tests/golden/long/hier_long100_n3.npz with the case machinery of make_golden.py (imported, not edited): the
REAL reference, Hierarchical with max_seq_len = 100 (paths of up to 100 commands, 102-token sequences), three icons of
eight groups from deepsvg_amd.synthetic.make_batch(3, 8, 100, ...): paths of mixed length, some longer than 62 commands,
and invisible groups.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_long.py

The fixture lives in a subdirectory: tests/helpers.golden_cases() runs every tests/golden/*.npz through the fixed-config
parity tests, whose config table has no long-path kind.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG        # noqa: E402

LONG_CASES = {"hier_long100_n3": ("hier_long100", 3, 5, 1234)}
_base_build_cfg = MG.build_cfg


def build_cfg(kind):
    if kind == "hier_long100":
        cfg = MG.ref_cfg.Hierarchical()
        cfg.use_vae = False
        cfg.max_seq_len = 100
        return cfg
    return _base_build_cfg(kind)


if __name__ == "__main__":
    MG.build_cfg = build_cfg
    MG.OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "long")
    os.makedirs(MG.OUT, exist_ok=True)
    for name in (sys.argv[1:] or LONG_CASES):
        MG.run_case(name, *LONG_CASES[name])
