"""Record tests/golden/profile_parent.npz, the expectation of tests/test_gpu_profile_parent.py, from a given build of the
library (the commit before the profiled fits shared one per-bin objective and one launch layer, built with the
toolchain the tests run under):

    PYTHONPATH=. python scripts/dev/record_profile_parent.py path/to/libpisa_hip.so [out.npz]

The cases, the seeds and what is kept of every output (arrays or digests) are the test module's own."""
import os
import sys

lib_path = os.path.abspath(sys.argv[1])
os.environ["PISA_HIP_LIB"] = lib_path      # read when pisa_amd._lib is imported

import numpy as np  # noqa: E402

from pisa_amd import _lib, kernels as K  # noqa: E402
from tests import test_gpu_profile_parent as t  # noqa: E402
from tests.test_gpu_prob3_join import toolchain  # noqa: E402

assert _lib.LIB_PATH == lib_path
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(t.__file__), "golden", t.FIXTURE)
rec = dict(t.fixture_header(), toolchain=np.array(toolchain()))
for group, run in t.groups():
    rec.update(t.to_fixture(group, run(K)))
np.savez_compressed(out, **rec)
print("%s: %d entries, %d bytes, from %s (%s)" % (out, len(rec), os.path.getsize(out), lib_path, rec["toolchain"]))
