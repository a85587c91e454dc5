"""
Worker for tests/test_framestats_cpu.py: one rank of a world_size-N gloo job that runs FEMUDF and LogsumUDF
(NumPy branch) through the HipJobExecutor's nav sharding and its merge across the ranks.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch.distributed as dist
    from libertem_amd.api import Context
    from libertem_amd.executor.hip import HipJobExecutor
    from libertem_amd.udf.FEM import FEMUDF
    from libertem_amd.udf.logsum import LogsumUDF

    out_dir = sys.argv[1]
    dist.init_process_group('gloo')
    rank = dist.get_rank()
    ctx = Context(executor=HipJobExecutor(require_gpu=False))
    rng = np.random.default_rng(78)
    data = rng.integers(0, 3000, (7, 9, 12, 13)).astype(np.uint16)
    ds = ctx.load('memory', data=data, num_partitions=7, sig_dims=2)
    fem = ctx.run_udf(dataset=ds, udf=FEMUDF(center=(6, 6), rad_in=2, rad_out=5))
    logsum = ctx.run_udf(dataset=ds, udf=LogsumUDF())
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), intensity=np.array(fem['intensity'].data),
             logsum=np.array(logsum['logsum'].data))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
