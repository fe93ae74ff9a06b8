"""Record tests/golden/prob3_join_parent.npz, the expectation of tests/test_gpu_prob3_join.py, from a given build of the
library (the commit before the two-sided join of the chain kernel, built with the toolchain the tests run under):

    PYTHONPATH=. python scripts/dev/record_prob3_join.py path/to/libpisa_hip.so [out.npz]

The cases and what is kept of them (arrays or digests) are the test module's own."""
import os
import sys

lib_path = os.path.abspath(sys.argv[1])
os.environ["PISA_HIP_LIB"] = lib_path      # read when pisa_amd._lib is imported

import numpy as np  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from pisa_amd import _lib, kernels as K  # noqa: E402
from tests import test_gpu_prob3_join as t  # noqa: E402

assert _lib.LIB_PATH == lib_path
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(t.__file__), "golden", t.FIXTURE)
orc.build()
setup = t.make_setup(K, orc)
rec = {"toolchain": np.array(t.toolchain())}
for n_e in t.N_ES:
    for e_major in (True, False):
        for name in t.NAMES:
            rec.update(t.to_fixture(t.one_point(K, setup, name, n_e, e_major)))
        rec.update(t.to_fixture(t.three_points(K, setup, n_e, e_major)))
np.savez_compressed(out, **rec)
print("%s: %d entries, %d bytes, from %s (%s)" % (out, len(rec), os.path.getsize(out), lib_path, rec["toolchain"]))
