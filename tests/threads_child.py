"""Child process of test_gpu_threads.py::test_first_use_from_four_threads: the process's very first library calls come
from four threads behind a barrier, each on a stream of its own and all with the same ring radius - erosion(Z, radius=18)
on one device tensor - so that the once-per-process launch-attribute caches are filled by four callers at once; then
one of the threads makes a springs solve.  stdout gets "erosion <thread> <digest>" four times and "springs <digest>".
The package is imported from the working directory."""
import hashlib
import os
import sys
import threading

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

RADIUS = 18
NTHREADS = 4
WAIT = 120.0


def inputs():
    import neilpy_amd
    Z = neilpy_amd.synth_dem(331, seed=11, rows=203).astype(np.float32)
    rng = np.random.default_rng(12)
    A = rng.normal(100.0, 5.0, (37, 53))
    A[rng.random(A.shape) < .5] = np.nan
    return Z, A


def digest(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    h = hashlib.sha1(str((a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def main():
    import torch
    import neilpy_amd
    Z, A = inputs()
    Zd, Ad = torch.from_numpy(Z).to("cuda:0"), torch.from_numpy(A).to("cuda:0")
    torch.cuda.synchronize()
    barrier = threading.Barrier(NTHREADS)
    lines, errors = [], []

    def body(t):
        try:
            stream = torch.cuda.Stream()
            barrier.wait(WAIT)
            with torch.cuda.stream(stream):
                lines.append("erosion %d %s" % (t, digest(neilpy_amd.erosion(Zd, radius=RADIUS))))
                barrier.wait(WAIT)
                if t == NTHREADS - 1:
                    assert neilpy_amd.inpaint_nans_by_springs(Ad, inplace=True) is None
                    lines.append("springs " + digest(Ad))
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))
            barrier.abort()
    threads = [threading.Thread(target=body, args=(t,)) for t in range(NTHREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    if errors or any(th.is_alive() for th in threads):
        print("errors", errors, file=sys.stderr)
        sys.stdout.flush()
        os._exit(1)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
