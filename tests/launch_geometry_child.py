"""Child process of test_gpu_w50.py::test_launch_geometry_is_asked_once_per_kernel: progressive_filter twice on a
64 x 600 fp32 raster with windows 1..16.  Under SMRF_FUSED=2 and SMRF_ERO_INC=2 (set by the parent, with SMRF_RING_DEBUG=1)
these are chained launches (windows 1..10), fused openings (11..14), two ring passes (15) and the incremental erosion (16):
all four marching launchers.  The library's geometry lines go to stderr; stdout gets one line, the digests of the two masks.
The package is imported from the working directory."""
import hashlib
import os
import sys

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

import neilpy_amd  # noqa: E402

Z = neilpy_amd.synth_dem(600, seed=7, rows=64)
windows = np.arange(1, 17)
masks = [neilpy_amd.progressive_filter(Z, windows, 1, .15) for _ in range(2)]
print("masks", *[hashlib.sha1(np.ascontiguousarray(m).tobytes()).hexdigest() for m in masks], int(masks[0].sum()))
