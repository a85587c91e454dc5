"""
What the UDFs that run on native plans share (crystallinity, correlation, holography, cepstrum, orientation: one plan
per frame shape, used by every tile; ssb, wdd, parallax: one plan per scan, used once per run): the plan cache and its
eviction rule, the workspace budget, the batch size of a frame plan, the device of a UDF, the digest of the arrays in
a cache key.
"""
import hashlib

#: workspace budget of one plan (f32 frames + complex64 half spectra of one batch), bytes.  Measured on 16 384 frames
#: of 256 x 256 (profiles/correlation.txt): batches of 32 / 128 / 255 / 1020 frames take 34.8 / 17.5 / 15.0 / 14.0 ms --
#: the transforms of a small batch do not fill the chip, and a batch that fits the Infinity Cache gains nothing
CORR_WORKSPACE_BYTES = 512 * 2**20

_OWNED = []          # the `owned` caches: what `release_device_plans` closes


class PlanCache(dict):
    """key -> native plan, at most `capacity` of them; key[0] is the device.  What happens to the plans when the
    cache is full, or the executor of their device closes, depends on who else may hold one:

    owned=True: nobody between two runs (the plan is used inside `get_results` only).  A full cache closes its plans
                (`release`): their HBM is free before the next plan allocates; `release_device_plans` closes them too.
    owned=False: kept task instances may (REUSE_TASK_INSTANCES).  A full cache only forgets its plans (`clear`); each
                 is destroyed with its last reference (`_NativePlan.__del__`), and closing an executor leaves them."""

    def __init__(self, capacity, owned):
        super().__init__()
        self.capacity, self.owned = int(capacity), bool(owned)
        if self.owned:
            _OWNED.append(self)

    def get_or_make(self, key, make):
        plan = self.get(key)
        if plan is None:
            if len(self) >= self.capacity:
                if self.owned:
                    self.release()
                else:
                    self.clear()
            plan = self[key] = make()
        return plan

    def release(self, device=None):
        """close and forget the plans of `device` (None: of every device)"""
        for key in [k for k in self if device is None or k[0] == int(device)]:
            self.pop(key).close()


def release_device_plans(device):
    """Close the plans of `device` in every owned cache and free their HBM: the HIP executor of that device closes."""
    for cache in _OWNED:
        cache.release(device)


def udf_device(udf):
    """the device a UDF's tiles live on"""
    return udf.meta.gpu_id if udf.meta.gpu_id is not None else 0


def frame_batch(udf, per_frame_bytes, budget):
    """frames per execution of a frame plan: as many as the workspace budget, the tile depth and the partition allow"""
    depth = int(udf.meta.tiling_scheme.depth) if udf.meta.tiling_scheme is not None else 1
    return max(1, min(budget // per_frame_bytes, depth, int(udf.meta.partition_shape[0])))


def array_digest(*arrays):
    """one hex digest of the bytes of `arrays` (None: skipped) for a cache key; each array is preceded by its position
    and length, so (a, b) and (a + b,) differ, as do (a, None) and (None, a)"""
    digest = hashlib.sha1()
    for i, a in enumerate(arrays):
        if a is not None:
            data = a.tobytes()
            digest.update(b'%d:%d:' % (i, len(data)))
            digest.update(data)
    return digest.hexdigest()
