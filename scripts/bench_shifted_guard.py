"""What shifted masks cost through `ltmi_apply_masks_shifted_host`: frames of 256 x 256 against 16 float32 masks (the
shape of the bench's ring stack), a descan correction of +-2 pixels (25 distinct shifts) and one constant shift;
uint16 frames (never guarded) and float32 frames (clean: the non-finite guard lists nothing; 1 % of the frames with a
NaN in a row the shift cuts off: those are computed again), written and accumulated.  HIP-event median of 10 calls.

    python scripts/bench_shifted_guard.py [n_frames]                       one library (LTMI_LIB, LTMI_NONFINITE_GUARD)
    python scripts/bench_shifted_guard.py --compare PARENT_LIB [repeats]   parent and this tree's library alternating
                                                                           (parent 1, new 1, parent 2, ...), every
                                                                           repeat a process of its own, then a table
"""
import os, re, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"shifted (.+?) +(\d+) frames: +([\d.]+) ms +\[(.*)\]")


def measure(n):
    import torch
    sys.path.insert(0, ROOT)
    from libertem_amd import hip
    sig, n_masks = (256, 256), 16
    n_px = sig[0] * sig[1]
    rng = np.random.default_rng(5)
    masks = (rng.random((n_masks, n_px)) - 0.25).astype(np.float32)
    descan = rng.integers(-2, 3, (n, 2)).astype(np.int32)
    constant = np.tile(np.array([[2, -1]], dtype=np.int32), (n, 1))
    h = hip.MaskHandle.dense(0, masks, np.float32)
    out = torch.zeros((n, n_masks), device='cuda', dtype=torch.float32)

    def timed(t, dt, shifts, acc, reps=10):
        def call():
            h.apply_shifted_host(t.data_ptr(), dt, n, n_px, sig[0], sig[1], shifts, out.data_ptr(), n_masks, acc)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times))

    u16 = torch.from_numpy(rng.integers(0, 4096, (n, n_px)).astype(np.uint16).view(np.int16)).cuda()   # (torch has no uint16 on the device)
    f32 = torch.rand((n, n_px), device='cuda')
    nan = f32.clone()
    nan[::100, 0] = float('nan')            # row 0 is cut off by every shift with dy > 0
    for name, t, dt in (('uint16', u16, np.uint16), ('float32 clean', f32, np.float32),
                        ('float32 1% NaN', nan, np.float32)):
        for sname, shifts in (('descan +-2', descan), ('constant', constant)):
            for acc in (False, True):
                ms = timed(t, dt, shifts, acc)
                print(f"shifted {name:15s} {sname:11s} {'accumulate' if acc else 'write     '} {n} frames: {ms:8.3f} ms   "
                      f"[{h.last_kernel()}]", flush=True)
    h.close()


def one_process(lib, guard_off=False):
    env = dict(os.environ)
    env.pop('LTMI_LIB', None)
    env.pop('LTMI_NONFINITE_GUARD', None)
    if lib:
        env['LTMI_LIB'] = lib
    if guard_off:
        env['LTMI_NONFINITE_GUARD'] = '0'
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300, check=True)
    res = {}
    for line in r.stdout.splitlines():
        m = LINE.match(line)
        if m:
            res[re.sub(r' +', ' ', m.group(1).strip())] = (float(m.group(3)), m.group(4))
    return res


def compare(parent_lib, repeats):
    par, new = [], []
    for _ in range(repeats):
        par.append(one_process(parent_lib))
        new.append(one_process(None))
    off = one_process(None, guard_off=True)
    print(f"{'case':44s} {'parent repeats (ms)':27s} {'new repeats (ms)':27s} parent spread   overhead (ms, %)   guard off (ms)")
    for k in par[0]:
        p, n = [r[k][0] for r in par], [r[k][0] for r in new]
        pm, nm = float(np.median(p)), float(np.median(n))
        print(f"{k:44s} {' '.join(f'{x:8.3f}' for x in p):27s} {' '.join(f'{x:8.3f}' for x in n):27s} "
              f"{max(p) - min(p):8.3f}      {nm - pm:+8.3f} {100 * (nm - pm) / pm:+6.1f} %   {off[k][0]:8.3f}")
    print("\nroutes (last_kernel), parent | new:")
    for k in new[0]:
        print(f"{k:44s} {par[0][k][1]} | {new[0][k][1]}")


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--compare':
        compare(os.path.abspath(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    else:
        measure(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
