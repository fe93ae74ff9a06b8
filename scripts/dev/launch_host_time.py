"""host time of the three C-ABI calls of one headline evaluation (they are asynchronous: this is what the host spends
issuing them) and of the Python around them"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ctypes as C
import numpy as np, torch
from pisa_amd import synthetic, _lib, kernels as K

wl = synthetic.Workload(n_events=10_000_000, grid=(200, 100), out_binning="dragon", seed=0)
st = synthetic.DeviceState(wl, compact=True)
p = wl.osc_params()
st.make_pseudo_data(p)
if len(sys.argv) > 1 and sys.argv[1] == "lean":   # the separate launches instead of the one-call evaluator
    st.one_call = False
for _ in range(20):
    st.eval_host(p)
a = st._arg_block()
lib, s = a["lib"], K._stream()
h = st._metric_host_np
T = np.zeros(5)
N = 300
for _ in range(N):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.pisa_hip_prob3_grid_planned(C.byref(p), a["plan"], a["energy"], a["n_e"], a["e_major"], None, None, a["pepmu"], s)
    t1 = time.perf_counter()
    rc |= st._launch_acc(a, a["nu"], a["nubar"], a["pepmu"])
    t2 = time.perf_counter()
    h[:] = np.nan
    n_parts = st._launch_tail("llh", None, st.TAIL_PARTS)
    t3 = time.perf_counter()
    v = float(st._join_parts(st._wait(h[:n_parts])))
    t4 = time.perf_counter()
    assert rc == 0
    T += [t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0]
T = T / N * 1e6
print("prob3_grid_planned %.2f us, accumulation %.2f us, tail %.2f us, poll until the value %.2f us, total %.2f us" % tuple(T))
t0 = time.perf_counter()
for _ in range(N):
    st.eval_host(p)
print("eval_host %.2f us per evaluation" % ((time.perf_counter() - t0) / N * 1e6))
