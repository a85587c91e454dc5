"""
Worker for tests/test_wsum_cpu.py: one rank of a world_size-N gloo job that runs WeightedSumUDF (NumPy branch)
through the HipJobExecutor's nav sharding; 'wsum' merges by 'sum' across the ranks.
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
    from libertem_amd.udf.weightedsum import WeightedSumUDF

    out_dir = sys.argv[1]
    dist.init_process_group('gloo')
    rank = dist.get_rank()
    ctx = Context(executor=HipJobExecutor(require_gpu=False))
    rng = np.random.default_rng(78)
    data = rng.integers(0, 3000, (7, 9, 12, 13)).astype(np.uint16)
    weights = rng.standard_normal((7, 9, 5)).astype(np.float32)
    roi = rng.random((7, 9)) > 0.5
    ds = ctx.load('memory', data=data, num_partitions=7, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(weights))
    res_roi = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(weights), roi=roi)
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), wsum=np.array(res['wsum'].data),
             roi_wsum=np.array(res_roi['wsum'].data))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
