"""Generate tests/golden/reference_pins.npz: the answers of the reference's own std-only headers on the seeded inputs of
tests/reference_pins.py, through oracle/_ref/libref.so (oracle/Makefile `ref`, which needs the reference's sources).

Unlike tests/golden/oracle_r01.json these ARE reference outputs: the tests that pin the restatement against the
reference's KD-tree, GridFilter, UnionFind, KMeans, Hilbert curve, interleave and unordered_dense read them, so they run
wherever the repository is checked out.

Run from the repository root:  make -C oracle ref && python scripts/make_reference_pins.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_pins as rp  # noqa: E402
from opencalibration_amd import synth  # noqa: E402  (data generators only)
from oracle import pyoracle  # noqa: E402


def main():
    out = rp.record(pyoracle, synth)
    np.savez_compressed(rp.GOLDEN, **out)
    print("wrote", rp.GOLDEN, len(out), "arrays,", os.path.getsize(rp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
