"""Child process of tests/test_rowdot_exact_gpu.py: row sums on more distinct streams than the process has ticket slots (32, shared
with tet_energies, never recycled).  The first 32 (device, stream) pairs take the one-launch ticket form, every later one the
two-launch form; all of them must give the exact sums, bit for bit those of the default stream.  Prints `ok: N streams`."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402

SLOTS = 32                                                      # restated from reduce.hip (kTicketSlots)
ROWS, WIDTH = 4, 131_073


def runtime_streams(count):
    """streams made by the HIP runtime that torch already has mapped, wrapped for torch (they live as long as the process)"""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    out = []
    for _ in range(count):
        handle = ctypes.c_void_p()
        status = hip.hipStreamCreate(ctypes.byref(handle))
        assert status == 0 and handle.value, "hipStreamCreate failed (%d)" % status
        out.append(torch.cuda.ExternalStream(handle.value))
    return out


def main():
    from deftet_amd import hip_ops
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(33)
    a, b = (rng.integers(-3, 4, (ROWS, WIDTH)).astype(np.int32) for _ in range(2))
    roots = rng.integers(0, 6, (ROWS, WIDTH)).astype(np.int32)
    assert np.abs(a * b).sum(1, dtype=np.int64).max() < 2**24 and roots.sum(1, dtype=np.int64).max() < 2**24
    want_dot = (a * b).sum(1, dtype=np.int64).astype(np.float64)
    want_sqrt = roots.sum(1, dtype=np.int64).astype(np.float64)
    ta, tb, tx = (torch.from_numpy(t.astype(np.float32)).to(dev) for t in (a, b, roots * roots))

    def run():
        return hip_ops.rowdot(ta, tb), hip_ops.sqrt_rowsum(tx, 0.0)

    def check(got, label):
        torch.cuda.synchronize()
        assert np.array_equal(got[0].double().cpu().numpy(), want_dot), "rowdot on %s" % label
        assert np.array_equal(got[1].double().cpu().numpy(), want_sqrt), "sqrt_rowsum on %s" % label
        assert all(torch.equal(g.view(torch.int32), f.view(torch.int32)) for g, f in zip(got, first)), "bits on %s" % label

    main_stream = torch.cuda.current_stream(dev)
    first = run()
    check(first, "the default stream")
    seen = {(dev.index, main_stream.cuda_stream)}
    streams = []
    for priority in (0, -1):                                    # torch hands out its pooled streams round robin, per priority
        for _ in range(2 * SLOTS):
            s = torch.cuda.Stream(device=dev, priority=priority)
            if (s.device.index, s.cuda_stream) not in seen:
                seen.add((s.device.index, s.cuda_stream))
                streams.append(s)
    while len(seen) < SLOTS + 4:
        for s in runtime_streams(SLOTS + 4 - len(seen)):
            if (s.device.index, s.cuda_stream) not in seen:
                seen.add((s.device.index, s.cuda_stream))
                streams.append(s)
    assert len(seen) >= SLOTS + 1

    def on(stream):
        stream.wait_stream(main_stream)
        with torch.cuda.stream(stream):
            got = run()
        main_stream.wait_stream(stream)
        return got

    for i, s in enumerate(streams):                             # stream 32 and later find the table full
        check(on(s), "side stream %d" % (i + 1))
    check(run(), "the default stream after the table is full")
    check(on(streams[0]), "the first side stream after the table is full")
    check(on(streams[SLOTS - 1]), "the first stream past the table, again")
    print("ok: %d streams" % len(seen))


if __name__ == "__main__":
    main()
