"""One fixed sequence of library calls over every per-device scratch buffer an evaluation step
touches, for tests/test_gpu_scratch.py: a fused-chain batched apply (40 states, 8 qubits,
capacity 64), overlaps, Hamming-weight-1 amplitudes, the flag check, a gradient sweep, a pair-RDM
sweep and an arg-max.  Run as a script it is the child process of the finalize-and-reuse test."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, CAP, NS = 8, 64, 40
PAIRS = [(a, b) for a in range(N) for b in range(a + 1, N)]


def scratch_stats():
    """[device bytes held, pinned bytes held, device allocations, pinned allocations]."""
    from adaptaqc_amd import _lib

    out = (ctypes.c_double * 4)()
    _lib.check(_lib.lib().aqc_scratch_stats(out))
    return list(out)


def handles(states):
    return (ctypes.c_void_p * len(states))(*[s.h.value for s in states])


def pair_rdms_batch(states, pairs):
    """[nstates, npairs, 4, 4] through aqc_mps_pair_rdms_batch (host output)."""
    from adaptaqc_amd import _lib

    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
    out = np.zeros(len(states) * (len(p) // 2) * 16, dtype=np.complex128)
    _lib.check(_lib.lib().aqc_mps_pair_rdms_batch(handles(states), len(states), _lib.ptr(p), len(p) // 2,
                                                  _lib.ptr(out), 0))
    return out.reshape(len(states), len(p) // 2, 4, 4)


def argmax_scaled(scores, prio):
    from adaptaqc_amd import _lib

    s = np.ascontiguousarray(scores, dtype=np.float64)
    p = np.ascontiguousarray(prio, dtype=np.float64)
    best = ctypes.c_int()
    _lib.check(_lib.lib().aqc_argmax_scaled(_lib.ptr(s), _lib.ptr(p), len(s), 0, ctypes.byref(best)))
    return best.value


def random_unitary_ops(n, layers, seed):
    """Brickwork of random two-qubit unitaries as an ops array."""
    from adaptaqc_amd import _lib

    rng = np.random.default_rng(seed)
    ops = []
    for layer in range(layers):
        for q in range(layer % 2, n - 1, 2):
            a = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
            ops.append((np.linalg.qr(a)[0], (q, q + 1)))
    return _lib.ops_array(ops)


class Sequence:
    def __init__(self):
        import bench
        from adaptaqc_amd.device import OpsBatch

        self.ops = OpsBatch([random_unitary_ops(N, 4, 500 + s) for s in range(NS)])
        _, _, self.deg, self.u0, self.gm = bench.layer_inputs()
        self.svec = np.zeros((N, 2), complex)
        self.svec[:, 0] = 1.0
        self.prio = np.random.default_rng(3).choice([0.5, 1.0], len(PAIRS))

    def run(self):
        """Fresh handles, the seven calls, handles closed again; every result as an array."""
        from adaptaqc_amd.device import (DeviceMPS, amps_hw1_batch, apply_batch, check_batch, overlap_zero_batch,
                                         pair_grads_batch)

        states = [DeviceMPS(N, CAP, 1e-16, CAP) for _ in range(NS)]
        try:
            apply_batch(states, self.ops, sort=True)
            out = {"overlap": overlap_zero_batch(states), "amps": amps_hw1_batch(states)}
            check_batch(states)
            out["grads"] = pair_grads_batch(states, self.svec, PAIRS, self.u0, self.gm, self.deg)
            out["rdms"] = pair_rdms_batch(states, PAIRS)
            out["best"] = np.array([argmax_scaled(out["grads"][0], self.prio)])
        finally:
            for s in states:
                s.close()
        return out


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def main():
    """The sequence, every handle closed, aqc_finalize, the sequence again: nothing held after the
    finalize, the same results bit for bit after it."""
    from adaptaqc_amd import _lib

    seq = Sequence()
    first = seq.run()
    held = scratch_stats()
    assert held[0] > 0 and held[1] > 0, held
    _lib.check(_lib.lib().aqc_finalize())
    after = scratch_stats()
    assert after[0] == 0 and after[1] == 0, after
    second = seq.run()
    assert same(first, second), [k for k in first if not np.array_equal(first[k], second[k])]
    assert np.max(first["grads"]) > 1e-6 and abs(first["overlap"]).max() > 1e-6  # (not all zero)
    print("scratch-sequence-ok")


if __name__ == "__main__":
    main()
