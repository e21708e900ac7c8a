"""The MPS measurements of csrc/mps_meas.hip where the other suites do not reach: the zero and
Hamming-weight-1 chains past their first 64-column block (bonds 64 -> 100 -> 100 -> 64: a partial
second block, row counts that are no multiple of the four waves) against the oracle, states of
different capacities in one batched call (the dynamic LDS is sized by the largest), a batched
read straight behind queued gate work (the job staging takes a set of the ring, it does not drain
the stream), and the windowed rows on a second device in one process (the kernels' dynamic-LDS
limit is raised per device)."""

import numpy as np
import pytest

from conftest import to_circuit
from oracle import mps as M

pytestmark = pytest.mark.gpu

_N = 15
_CACHE = {}


def _vidal(chi, seed):
    """bench.random_vidal_mps(15, chi, seed), built once per (chi, seed)"""
    import bench

    if (chi, seed) not in _CACHE:
        _CACHE[chi, seed] = bench.random_vidal_mps(_N, chi, seed)
    return _CACHE[chi, seed]


def _state(cap, chi, seed):
    from adaptaqc_amd.device import DeviceMPS

    d = DeviceMPS(_N, cap, 1e-16, cap)
    d.load_aer(_vidal(chi, seed))
    return d


def _dops(n, ops):
    from adaptaqc_amd.circuit import device_ops

    return device_ops(to_circuit(n, ops))


def test_ragged_wide_bonds_vs_oracle():
    """15 qubits at capacity 128 with bonds .., 64, 100, 100, 64, ..: <psi|0> and every <e_i|psi>
    against the oracle's contractions of the read-back state at 1e-12 (the tolerance of
    test_gpu_zsum.py for these quantities), and the single-state amplitudes bit for bit the batched
    call's row."""
    from adaptaqc_amd.device import amps_hw1_batch

    d = _state(128, 100, 11)
    assert list(d.dims()[6:10]) == [64, 100, 100, 64]
    pre = d.preprocessed()
    assert abs(d.overlap_zero() - M.mps_dot(pre, M.zero_mps(_N))) < 1e-12
    amps = d.amps_hw1()
    np.testing.assert_allclose(amps, [M.extract_amplitude(pre, 2 ** i) for i in range(_N)], rtol=0, atol=1e-12)
    other = _state(128, 100, 12)
    assert np.array_equal(amps_hw1_batch([other, d])[1], amps)


def test_mixed_capacities_in_one_batch():
    """Capacities 16 and 128 in one overlap_zero_batch and one amps_hw1_batch call: every row bit for
    bit the single-state call's."""
    from adaptaqc_amd.device import amps_hw1_batch, overlap_zero_batch

    states = [_state(16, 16, 21), _state(128, 100, 11), _state(128, 100, 12), _state(16, 16, 22)]
    ov = overlap_zero_batch(states)
    amps = amps_hw1_batch(states)
    for k, d in enumerate(states):
        assert ov[k] == d.overlap_zero()
        assert np.array_equal(amps[k], d.amps_hw1())


def test_amps_behind_queued_gates_without_a_drain():
    """apply_batch(wait=False) and amps_hw1_batch at once (the states come out sorted, so the call
    queues its launches behind the gate work without waiting for it): bit for bit the amplitudes of
    four identically prepared states applied with wait=True.  Then check_batch."""
    import bench
    from adaptaqc_amd.device import DeviceMPS, amps_hw1_batch, apply_batch, check_batch

    n, cap = 8, 16
    rng = np.random.default_rng(5)
    lists = []
    for s in range(4):
        ops = []
        for layer in range(3):
            for q in range(n):
                ops.append(("ry", (q,), (float(rng.uniform(-np.pi, np.pi)),)))
            for q in range(layer % 2, n - 1, 2):
                ops.append(("cx", (q, q + 1), ()))
        ops.append(("cx", (0, n - 1), ()))  # (routed: the sort has swaps to undo)
        lists.append(_dops(n, ops))

    def prepared():
        out = []
        for s in range(4):
            d = DeviceMPS(n, cap, 1e-16, cap)
            d.load_aer(bench.random_vidal_mps(n, 8, 40 + s))
            out.append(d)
        return out

    waited, queued = prepared(), prepared()
    apply_batch(waited, lists, sort=True, wait=True)
    want = amps_hw1_batch(waited)
    apply_batch(queued, lists, sort=True, wait=False)
    got = amps_hw1_batch(queued)
    check_batch(queued)
    assert np.abs(want).max() > 1e-3
    assert np.array_equal(got, want)


def test_windowed_rows_on_a_second_device():
    """zero_hw1_batch(base, cands, amps=True) at 6 qubits, capacity 64 (72.7 KB of dynamic LDS in
    k_hw_win, above the 64 KB default) on device 0 and then, in the same process, with handles
    created under device 1: both against the oracle at 1e-12."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    import bench
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS, copy_batch, zero_hw1_batch

    n, cap = 6, 64
    rng = np.random.default_rng(9)
    lists = [_dops(n, [("ry", (a, ), (float(rng.uniform(-np.pi, np.pi)),)), ("cx", (a, a + 1), ())]) for a in (1, 3)]
    lib = _lib.lib()
    home = _lib.device_index()

    def run():
        base = DeviceMPS(n, cap, 1e-16, cap)
        base.load_aer(bench.random_vidal_mps(n, 8, 60))
        cands = [DeviceMPS(n, cap, 1e-16, cap) for _ in lists]
        copy_batch(cands, [base] * len(cands))
        for d, ops in zip(cands, lists):
            d.apply(ops)
        ov, amps = zero_hw1_batch(base, cands, amps=True)
        for k, d in enumerate(cands):
            pre = d.preprocessed()
            assert abs(ov[k] - M.mps_dot(pre, M.zero_mps(n))) < 1e-12
            np.testing.assert_allclose(amps[k], [M.extract_amplitude(pre, 2 ** i) for i in range(n)], rtol=0, atol=1e-12)
        for d in cands + [base]:
            d.close()

    other = 1 if home != 1 else 0
    run()
    _lib.check(lib.aqc_init(other))
    try:
        run()
    finally:
        _lib.check(lib.aqc_init(home))
