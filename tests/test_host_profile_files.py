"""bench.py reads the newest committed profiles/r*/kernels_by_phase.json and traffic.json (`trace_roofline`,
`pmc_traffic`): whatever round is the newest, the two files hold what those functions take from them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_newest_kernel_trace_file_has_the_accumulate_kernel_time():
    import bench

    d, src = bench.latest_profile("kernels_by_phase.json")
    assert d is not None and os.path.isdir(os.path.join(ROOT, src))
    us = d["hist_accumulate_kernel"]["timed_loop_mean_us"]
    assert isinstance(us, float) and 0.0 < us < 1e6


def test_newest_traffic_file_has_the_hbm_bytes():
    import bench

    d, src = bench.latest_profile("traffic.json")
    assert d is not None and os.path.isdir(os.path.join(ROOT, src))
    assert isinstance(d["hbm_bytes"], float) and d["hbm_bytes"] > 0.0
