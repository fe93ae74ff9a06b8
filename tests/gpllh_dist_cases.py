"""Ranks of tests/test_gpu_gpllh.py's multi-rank case, started through `torch.distributed.run`:

    python -m torch.distributed.run --nproc-per-node N ... tests/gpllh_dist_cases.py <out_dir>

Every rank on HIP device 0, exchanging over gloo (the one-GPU stand-in of one rank per GPU, as in
tests/test_gpu_distributed.py): the synthetic low-MC workload sharded over the ranks, `configure_gpllh` (the MC counts
all-reduced), then the generalized likelihood at three points through `eval_host` and `eval_many`; every rank writes
its values (float.hex) and the MC count table it configured."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(out_dir):
    import numpy as np
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    group = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=20000, grid=(24, 16), out_binning="dragon", seed=3)
    st = synthetic.DeviceState(wl, rank=rank, world_size=world, group=group)
    p = wl.osc_params(theta23_deg=45.0, dm31=2.4e-3)
    st.accumulate(p)
    st.allreduce()
    st.finalize()
    t = st.ws.hist.sum(dim=0).cpu().numpy()
    st.set_data(np.floor(t * (300.0 / t.max())))
    n_mc, _ = st.configure_gpllh()
    pts = [wl.osc_params(theta23_deg=a, dm31=b) for a, b in ((45.0, 2.4e-3), (42.0, 2.5e-3), (48.5, 2.3e-3))]
    values = [st.eval_host(q, "generalized_poisson_llh") for q in pts]
    many = st.eval_many(pts, "generalized_poisson_llh")
    st.check_status()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "gpllh_r%d.json" % rank), "w") as fh:
        json.dump({"rank": rank, "world": world, "n_mc": n_mc.tolist(), "values": [float(v).hex() for v in values],
                   "many": [float(v).hex() for v in many]}, fh)
    st.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
