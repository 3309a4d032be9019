#!/usr/bin/env python3
"""Write tests/golden/rd_search_samples.npz from the REAL reference (oracle/_ref/libalp_ref.so): the built sample sets of
tests/rd_search_inputs.py and the reference's cut, dictionary, estimate and sorted list for each (tests/rd_search_golden.py).
Runs only where the reference is built; the fixture is data and travels to the GPU machine, where the reference does not exist."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.pyoracle import Reference, ReferenceF32  # noqa: E402
import rd_search_golden  # noqa: E402

if __name__ == "__main__":
    arrays = rd_search_golden.record({64: Reference(), 32: ReferenceF32()})
    np.savez_compressed(rd_search_golden.PATH, **arrays)
    print(rd_search_golden.PATH, os.path.getsize(rd_search_golden.PATH), "bytes")
