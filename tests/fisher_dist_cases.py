"""Ranks of tests/test_gpu_fisher.py's multi-rank case, started through `torch.distributed.run`:

    python -m torch.distributed.run --nproc-per-node N ... tests/fisher_dist_cases.py <out_dir>

Every rank on HIP device 0, exchanging over gloo (the one-GPU stand-in of one rank per GPU, as in
tests/test_gpu_distributed.py): the synthetic workload sharded over the ranks, then `fisher_many` at P = 8 (17 points,
two sweeps); every rank writes the matrix and a digest of the gradients (float.hex)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(out_dir):
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    group = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=12 * 5003, grid=(24, 16), out_binning="dragon", seed=3)
    st = synthetic.DeviceState(wl, rank=rank, world_size=world, group=group, compact=True)
    pts, pairs, dx = [wl.osc_params()], [], []
    for p in range(8):
        th, dm = 40.0 + 0.5 * p, 2.4e-3 + 1e-5 * p
        pts += [wl.osc_params(theta23_deg=th + 1.0, dm31=dm), wl.osc_params(theta23_deg=th - 1.0, dm31=dm + 2e-5)]
        pairs.append((2 + 2 * p, 1 + 2 * p))
        dx.append(1.0 + 0.25 * p)
    res = st.fisher_many(pts, pairs, dx)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "fisher_r%d.json" % rank), "w") as fh:
        json.dump({"rank": rank, "world": world, "sweeps": res["sweeps"],
                   "matrix": [float(v).hex() for v in res["matrix"].cpu().numpy().ravel()],
                   "grad": [float(v).hex() for v in res["grad"].cpu().numpy().ravel()]}, fh)
    st.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
