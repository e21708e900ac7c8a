"""The per-device scratch buffers of the host-side staging (aqc::DevScratch / PerDevice tables,
csrc/aqc_internal.h) under growth, in steady state and across aqc_finalize.

Every test starts from empty tables (aqc_finalize releases them; handles that other modules keep
own their memory and streams and are not affected), so a family's first call allocates, its large
call regrows -- seen in aqc_scratch_stats' allocation counts -- and its third call, the first one
repeated, allocates nothing and returns the first result bit for bit.  References and tolerances
are those of each family's own tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sampling_ref as sref
import scratch_sequence as seq
import tomography_ref as tref
from conftest import to_circuit
from oracle import adapt_host
from oracle import entanglement as OE
from oracle import gradients as ogr
from oracle import mps as M

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def empty_tables():
    from adaptaqc_amd import _lib

    _lib.check(_lib.lib().aqc_finalize())
    st = seq.scratch_stats()
    assert st[0] == 0 and st[1] == 0, st


def allocations(stats):
    return stats[2] + stats[3]


def small_large_small(call, small, large, check):
    """call(small), call(large), call(small): allocations on the first two, none on the third;
    check(argument, result) on each; the first and third results bit for bit."""
    s0 = seq.scratch_stats()
    first = call(small)
    s1 = seq.scratch_stats()
    big = call(large)
    s2 = seq.scratch_stats()
    third = call(small)
    s3 = seq.scratch_stats()
    assert allocations(s1) > allocations(s0) and allocations(s2) > allocations(s1), (s0, s1, s2)  # regrown
    assert s3[2:] == s2[2:], (s2, s3)
    check(small, first)
    check(large, big)
    check(small, third)
    assert np.array_equal(first, third)


# ---- 1. small, large, small ----------------------------------------------------------------------
def test_argmax_grows_and_shrinks():
    def inputs(count):
        rng = np.random.default_rng(count)
        return rng.integers(0, 4, count).astype(float), rng.choice([-1.0, 0.5, 1.0], count)

    def check(arg, got):
        assert got == int(np.argmax(arg[0] * arg[1]))

    small_large_small(lambda a: seq.argmax_scaled(*a), inputs(5), inputs(5000), check)


def test_sample_uniforms_grows_and_shrinks():
    from adaptaqc_amd.device import sample_uniforms

    def check(shape, got):
        assert np.array_equal(got, sref.uniforms(2 ** 40 + 3, 5, *shape))

    small_large_small(lambda s: sample_uniforms(2 ** 40 + 3, 5, *s), (4, 3), (600, 500), check)


def _random_rdms(count, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((count, 4, 4)) + 1j * rng.standard_normal((count, 4, 4))
    rho = g @ g.conj().transpose(0, 2, 1)
    return rho / np.trace(rho, axis1=1, axis2=2)[:, None, None]


def test_pair_tomo_probs_host_path_grows_and_shrinks():
    from adaptaqc_amd.device import pair_tomo_probs

    def check(rdms, got):
        np.testing.assert_allclose(got, tref.pair_tomo_probs(rdms), atol=1e-13, rtol=0)

    small_large_small(pair_tomo_probs, _random_rdms(1, 1), _random_rdms(5000, 2), check)


def test_sv_pauli_grows_and_shrinks():
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceSV
    from test_gpu_pauli import random_labels, sv_pauli_ref

    def state(n, nterms):
        d = DeviceSV(n)
        d.apply(device_ops(to_circuit(n, sref.brickwork(n, 4, 100 + n))))
        return d, d.get(), random_labels(n, nterms, 7 + n)

    def check(arg, got):
        _, psi, labels = arg
        np.testing.assert_allclose(got, [sv_pauli_ref(psi, l) for l in labels], rtol=0, atol=1e-11)

    small_large_small(lambda a: a[0].pauli_expect(a[2]), state(4, 3), state(12, 400), check)


_MPS_N, _MPS_CAP = 8, 8
_MPS_REF = {}


def _mps_batch(seeds):
    """Random chi = 8 states of 8 qubits on the device, and the oracle's overlaps, Hamming-weight-1
    amplitudes, <Z_i> and pair RDMs of each (computed once per seed)."""
    import bench
    from adaptaqc_amd.device import DeviceMPS

    n = _MPS_N
    states, ref = [], {"overlap": [], "amps": [], "z": [], "rdms": []}
    for s in seeds:
        q = bench.random_vidal_mps(n, _MPS_CAP, 700 + s)
        d = DeviceMPS(n, _MPS_CAP, 1e-16, _MPS_CAP)
        d.load_aer(q)
        states.append(d)
        if s not in _MPS_REF:
            pre = M.MPS.from_aer(q).preprocessed()
            _MPS_REF[s] = {"overlap": M.mps_dot(pre, M.zero_mps(n)),
                           "amps": [M.extract_amplitude(pre, 1 << i) for i in range(n)],
                           "z": [M.mps_expectation_z(pre, i) for i in range(n)],
                           "rdms": [OE.mps_rdm(pre, a, b) for a, b in seq.PAIRS]}
        for k in ref:
            ref[k].append(_MPS_REF[s][k])
    return states, {k: np.array(v) for k, v in ref.items()}


@pytest.mark.parametrize("family", ["overlap", "amps", "check", "z", "rdms"])
def test_mps_batch_calls_grow_and_shrink(family):
    """aqc_mps_overlap_zero_batch, _amps_hw1_batch, _check_batch, _z_all_batch and the pair-RDM
    sweep on 2, 70 and 2 states of 8 qubits at capacity 8."""
    from adaptaqc_amd.device import amps_hw1_batch, check_batch, overlap_zero_batch, z_all_batch

    calls = {"overlap": overlap_zero_batch, "amps": amps_hw1_batch, "z": z_all_batch,
             "rdms": lambda st: seq.pair_rdms_batch(st, seq.PAIRS),
             "check": lambda st: np.array([check_batch(st) is None])}
    atol = {"amps": 1e-14, "z": 1e-12, "rdms": 1e-12}

    def check(arg, got):
        ref = arg[1]
        if family == "overlap":
            assert np.all(np.abs(got - ref["overlap"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["overlap"])) + 1e-30)
        elif family != "check":
            np.testing.assert_allclose(got, ref[family], rtol=0, atol=atol[family])

    small_large_small(lambda a: calls[family](a[0]), _mps_batch(range(2)), _mps_batch(range(70)), check)


_SVD_REF = {}


@pytest.mark.parametrize("gram", [1, 0], ids=["gram_big", "block_jacobi"])
def test_two_site_updates_at_256_grow_and_shrink(gram):
    """Two-site updates at 2 chi = 256 on the multi-workgroup Gram path and on the block Jacobi (the
    Gram path switched off): one job, three jobs in one wave, one job; each state against the oracle
    as test_gpu_gram_big.py checks its smallest size (bond dims exact, fidelity 1e-6)."""
    import bench
    from test_gpu_gram_big import _gates, _run

    n, chi, seed = 20, 128, 31
    jobs = {1: [(9, 10)], 3: [(7, 8), (9, 10), (11, 12)]}

    def run(nj):
        ops = _gates(n, np.random.default_rng(chi + nj), jobs[nj])
        d, st = _run(n, chi, ops, seed=seed, gram=gram)
        assert st["taken"] == (nj if gram else 0) and st["timeouts"] == 0, st
        if nj not in _SVD_REF:
            _SVD_REF[nj] = M.run_circuit(n, ops, 1e-16, chi, mps=M.MPS.from_aer(bench.random_vidal_mps(n, chi, seed)))
        pre_ref, pre = _SVD_REF[nj].preprocessed(), d.preprocessed()
        np.testing.assert_array_equal(d.dims(), [1] + [x.shape[2] for x in pre_ref])
        fid = abs(M.mps_dot(pre_ref, pre)) / np.sqrt(abs(M.mps_dot(pre, pre)) * abs(M.mps_dot(pre_ref, pre_ref)))
        assert abs(fid - 1.0) < 1e-6, fid
        return pre

    s0 = seq.scratch_stats()
    first = run(1)
    s1 = seq.scratch_stats()
    run(3)
    s2 = seq.scratch_stats()
    third = run(1)
    if not gram:  # (the block Jacobi's buffer is a DevScratch; the Gram path's arrays are its own)
        assert s1[2] > s0[2] and s2[2] > s1[2], (s0, s1, s2)
    assert seq.scratch_stats()[2:] == s2[2:]
    for a, b in zip(first, third):
        assert np.array_equal(a, b)


# ---- 2. the segmented sweep's cached plan across a regrow ------------------------------------------
def test_sweep_plan_cache_across_regrow():
    """The segmented single-state sweep keeps its last plan (job and pointer tables on the device)
    while the state and the pair list repeat.  A larger state regrows its scratch and must drop the
    plan: the first state swept again gives its first result bit for bit, a repeat (the plan
    reused) too, and every result matches oracle/gradients.py (1e-10, test_gpu_sweep_modes.py)."""
    import ctypes

    import bench
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS, pair_grads_batch

    _, _, deg, u0, gm = bench.layer_inputs()
    o_layer, o_gens, o_deg, o_inv = bench.oracle_layer()

    def state(n, chi, seed):
        q = bench.near_product_mps(n, chi, seed)
        d = DeviceMPS(n, 16, 1e-16, 16)  # (capacity 16: the smallest the segmented sweep takes)
        d.load_aer(q)
        cmap = adapt_host.coupling_map_full(n)
        svec = np.zeros((n, 2), complex)
        svec[:, 0] = 1.0
        want = ogr.general_grad_of_pairs_env(M.MPS.from_aer(q).preprocessed(), n, o_inv, o_gens, o_deg, cmap)
        assert np.max(want) > 1e-4
        return d, svec, cmap, want

    def sweep(s):
        got = pair_grads_batch([s[0]], s[1], s[2], u0, gm, deg)[0]
        np.testing.assert_allclose(got, s[3], rtol=0, atol=1e-10)
        return got

    small, large = state(8, 8, 41), state(16, 16, 42)
    assert len(small[2]) == 28
    L = _lib.lib()
    _lib.check(L.aqc_sweep_set_chain_mode(ctypes.c_int(3)))
    try:
        first = sweep(small)
        s1 = seq.scratch_stats()
        sweep(large)
        s2 = seq.scratch_stats()
        assert s2[2] > s1[2], (s1, s2)  # the segment scratch regrew
        third = sweep(small)
        again = sweep(small)
        assert seq.scratch_stats()[2:] == s2[2:]
    finally:
        _lib.check(L.aqc_sweep_set_chain_mode(ctypes.c_int(0)))
    assert np.array_equal(first, third) and np.array_equal(first, again)


# ---- 3. no allocation in steady state ------------------------------------------------------------
def test_no_allocation_in_steady_state():
    """The sequence of scratch_sequence.py four times (the longest ring has four sets), then twice
    more: no device or pinned allocation in the last two runs, and the same results."""
    s = seq.Sequence()
    runs = [s.run() for _ in range(4)]
    before = seq.scratch_stats()
    assert before[2] > 0 and before[3] > 0
    runs += [s.run() for _ in range(2)]
    after = seq.scratch_stats()
    assert after[2] == before[2] and after[3] == before[3], (before, after)
    for r in runs[1:]:
        assert seq.same(runs[0], r)


# ---- 4. finalize and reuse -----------------------------------------------------------------------
def test_finalize_releases_everything_and_the_library_works_again():
    """In a fresh interpreter (scratch_sequence.py as a script): the sequence, every handle closed,
    aqc_finalize -- no device or pinned scratch bytes held -- then new handles and the sequence
    again with the same results bit for bit."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scratch_sequence.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("scratch-sequence-ok")
