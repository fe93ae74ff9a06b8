#!/usr/bin/env python
"""Measure the figures the flux tests' bounds are built from (tests/flux_cases.py: G_REF, R_REF_HONDA, R_REF_BARTOL).

TEST INFRASTRUCTURE.  Run next to `gen_golden.py`, where the reference tree is at hand (oracle/ref_shim.py): the
Bartol residual is that of the reference's own `calculate_2d_flux_weights`; without the tree only the figures of
the C oracle and of oracle/flux_oracle.py are printed (tests/test_host_flux_cases.py holds those in every run).

    python oracle/measure_flux_refs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
import ref_shim  # noqa: E402
from oracle import oracle as _oracle  # noqa: E402
from pisa_amd.utils.resources import find_resource  # noqa: E402
from tests import flux_cases as fc  # noqa: E402

if __name__ == "__main__":
    print("Barr gate ratios, smallest |d|:", fc.barr_reference_ratios(_oracle))
    print("Honda r_ref (oracle): %.3g" % fc.oracle_preservation_residual(find_resource(fc.HONDA)))
    if ref_shim.available():
        fw = ref_shim.ref_module("pisa.utils.flux_weights")
        for name, table in (("honda", fc.HONDA), ("bartol", fc.BARTOL)):
            energy, bands = fc.read_table(find_resource(table))
            pts = fc.quadrature_points(name, energy)
            ee, cc = [a.ravel() for a in np.meshgrid(pts["e"], pts["cz"], indexing="ij")]
            splines = fw.load_2d_table(table)
            r = max(fc.preservation_residual(name, energy, bands[p], pts,
                                             fw.calculate_2d_flux_weights(ee, cc, splines[p]).reshape(pts["e"].size, -1))
                    for p in fc.TABLE_COLUMNS)
            print("%s r_ref (reference): %.3g" % (name, r))
