"""The MPS readers on loaded states whose bonds fill every workgroup's column slice of the split
environment chains (csrc/ent.hip: k_env_split<32 / 64 / 128> with 4 workgroups per chain at
capacities 128 / 256 / 512, k_env_split<64, 16> at 1024, and the Z-sum chains k_zenv on the same
table).  The other suites load small bonds into these capacities, so that only slice 0 owns any
column; the states of wide_mps_ref.py reach the capacity on one bond (every slice full), end
strictly inside upper slices on others and leave them empty on the rest (test_wide_mps_ref_host.py
proves that of the bond lists).

Every reader is compared with the host references of wide_mps_ref.py at the suite's bars (1e-11
against the oracle for <Z>, RDM entries, Z-sums and Pauli terms, 1e-12 for <psi|0>, amplitudes,
inner products and batch against single-state calls; n * chi * eps = 25 * 1024 * 1.1e-16 = 3e-12 of
accumulated rounding on O(1) quantities at the widest), and every call is bracketed by
aqc_env_fallbacks: a moved counter means a hand-off timed out and k_rdm_env, not the split kernel,
produced the values."""
import contextlib
import ctypes
import functools
import time

import numpy as np
import pytest

import sampling_ref as ref
import wide_mps_ref as W
from conftest import to_circuit
from oracle import mps as M

pytestmark = pytest.mark.gpu

ATOL = 1e-11  # against the oracle: test_gpu_ent.py, test_gpu_zsum.py, test_gpu_pauli.py
BATCH = 1e-12  # batch against single-state calls; <psi|0>, <e_i|psi>, <a|b> against the oracle
CAPS = [128, 256, 512, 1024]


def _fallbacks():
    from adaptaqc_amd import _lib

    cnt = ctypes.c_longlong(0)
    _lib.check(_lib.load().aqc_env_fallbacks(ctypes.byref(cnt)))
    return cnt.value


@contextlib.contextmanager
def split_only():
    """The split kernels answered: no environment launch inside timed out and was re-run."""
    before = _fallbacks()
    yield
    assert _fallbacks() == before, "a split chain timed out: k_rdm_env produced these values"


def loaded(cap, which=0):
    """(device state, oracle tensors) of wide_mps_ref.state(cap, which), once per module; the tests
    do not modify them."""
    return _loaded(cap, which)


def oracle_z(cap, which=0):
    return _oracle_z(cap, which)


@functools.lru_cache(maxsize=None)
def _loaded(cap, which):
    from adaptaqc_amd.device import DeviceMPS

    t0 = time.perf_counter()
    aer = W.state(cap, which)
    d = DeviceMPS(len(aer[0]), cap, 1e-16, None)
    d.load_aer(aer)
    assert list(d.dims()) == W.DIMS[cap]
    print(f"host: state {which} of capacity {cap} built and loaded in {time.perf_counter() - t0:.1f} s", flush=True)
    return d, W.preprocessed(aer)


@functools.lru_cache(maxsize=None)
def _oracle_z(cap, which):
    return W.oracle_z(loaded(cap, which)[1])


def _fresh(cap, which=0):
    """A new device state loaded with state(cap, which), for the tests that rewrite it."""
    from adaptaqc_amd.device import DeviceMPS

    aer = W.state(cap, which)
    d = DeviceMPS(len(aer[0]), cap, 1e-16, None)
    d.load_aer(aer)
    return d


def _dops(n, ops):
    from adaptaqc_amd.circuit import device_ops

    return device_ops(to_circuit(n, ops))


def _layer(rng, qubits):
    ops = []
    for q in qubits:
        ops.append(("ry", (q,), (float(rng.uniform(-np.pi, np.pi)),)))
        ops.append(("rz", (q,), (float(rng.uniform(-np.pi, np.pi)),)))
    return ops


def _report(reader, cap, dev):
    print(f"WIDE_PARITY {reader} cap {cap}: {dev:.2e}", flush=True)


@pytest.mark.parametrize("cap", CAPS)
def test_z_all_batch_vs_oracle(cap):
    """Every <Z_i> of two wide states of one bond list (one state at 1024, for the host time) in one
    batched call against the oracle's full contractions, and the batch row against z_all()."""
    from adaptaqc_amd.device import z_all_batch

    whichs = (0,) if cap == 1024 else (0, 1)
    states = [loaded(cap, w)[0] for w in whichs]
    with split_only():
        z = z_all_batch(states)
    dev = 0.0
    for row, w in zip(z, whichs):
        dev = max(dev, float(np.max(np.abs(row - oracle_z(cap, w)))))
    _report("z_all_batch", cap, dev)
    for row, w in zip(z, whichs):
        np.testing.assert_allclose(row, oracle_z(cap, w), rtol=0, atol=ATOL)
    with split_only():
        single = states[-1].z_all()
    np.testing.assert_allclose(z[-1], single, rtol=0, atol=BATCH)


@pytest.mark.parametrize("cap", CAPS)
def test_pair_rdms_vs_oracle(cap):
    """Pair RDMs around the widest bond (left of it, across it adjacent and at a distance, reversed,
    right of it, the chain's two ends) against the oracle's contraction; unit trace and Hermitian
    at the same bar.  At 1024 three distinct lower qubits (each runs k_rdm_chain through every wide
    bond to its right)."""
    d, pre = loaded(cap)
    k = W.widest(W.DIMS[cap])
    pairs = W.rdm_pairs(d.n, k, three_lowers=cap == 1024)
    assert len({min(p) for p in pairs}) <= (3 if cap == 1024 else 5)
    with split_only():
        rho = d.pair_rdms(pairs)
    want = W.oracle_rdms(pre, pairs)
    _report("pair_rdms", cap, float(np.max(np.abs(rho - want))))
    for p, r, w in zip(pairs, rho, want):
        np.testing.assert_allclose(r, w, rtol=0, atol=ATOL, err_msg=str(p))
        assert abs(np.trace(r) - 1.0) < ATOL, p
        np.testing.assert_allclose(r, r.conj().T, rtol=0, atol=ATOL, err_msg=str(p))


@pytest.mark.parametrize("cap", [512, 1024])
def test_every_slice_at_full_weight_left_canonical_gauge(cap):
    """In Vidal form the top slice of a wide bond holds the smallest Schmidt values (1e-5 of the
    weight at 512, 1e-8 at 1024): a slightly wrong top slice there moves <Z> by less than the bar.
    The same bond
    list in the left-canonical gauge with lambda = 1 (the readers contract A = Gamma lambda as
    loaded) spreads the weight evenly over the columns: <Z> of every site, the pair RDMs around the
    widest bond and the full Z-sum chains (k_zenv through every bond in both directions, the state
    being no copy of the prefix) against the oracle's contractions."""
    from adaptaqc_amd.device import DeviceMPS, z_all_batch, z_sum_batch

    aer = W.flat_state(cap)
    pre = W.preprocessed(aer)
    n = len(pre)
    d = DeviceMPS(n, cap, 1e-16, None)
    d.load_aer(aer)
    assert list(d.dims()) == W.DIMS[cap]
    want_z = W.oracle_z(pre)
    with split_only():
        z = z_all_batch([d])[0]
    _report("z_all_batch (left-canonical)", cap, float(np.max(np.abs(z - want_z))))
    np.testing.assert_allclose(z, want_z, rtol=0, atol=ATOL)
    pairs = W.rdm_pairs(n, W.widest(W.DIMS[cap]), three_lowers=True)
    with split_only():
        rho = d.pair_rdms(pairs)
    want = W.oracle_rdms(pre, pairs)
    _report("pair_rdms (left-canonical)", cap, float(np.max(np.abs(rho - want))))
    np.testing.assert_allclose(rho, want, rtol=0, atol=ATOL)
    with split_only():
        zs = z_sum_batch(loaded(cap)[0], [d])[0]
    _report("z_sum_batch (left-canonical, full chains)", cap, abs(zs - want_z.sum()))
    assert abs(zs - want_z.sum()) < ATOL


@pytest.mark.parametrize("cap", [256, 512, 1024])
def test_z_sum_windows_at_the_wide_bond(cap):
    """sum_i <Z_i> through windows on a wide prefix state: candidates copied from it and rewritten by
    (a) one-qubit gates on the two sites beside the widest bond (no SVD: the window's k_zenv steps
    run at the full width), (b) a cx with rotations across a bond of a few hundred two sites to the
    right, (c) nothing; and a state not copied from the prefix (the full chains through every wide
    bond in both directions).  Against z_all_batch's row sums, candidate (a) against the oracle's
    sum on its read-back tensors; then the prefix takes a one-qubit gate on a wide-bond site (its
    cached pairs are extended at width) and fresh candidates are checked again."""
    from adaptaqc_amd.device import DeviceMPS, copy_batch, z_all_batch, z_sum_batch

    dims = W.DIMS[cap]
    n, k = len(dims) - 1, W.widest(dims)
    m = k + 2  # the bond between sites m - 1 and m: 130 / 200 / 400, at most 2 * dims[m + 1] after the cx
    assert 100 <= dims[m] <= 400 and 2 * dims[m + 1] <= cap
    rng = np.random.default_rng(cap)
    base = _fresh(cap)
    other = _fresh(cap, 0 if cap == 1024 else 1)  # (not a copy of base to the library, whatever it holds)
    cands = [DeviceMPS(n, cap, 1e-16, None) for _ in range(3)]

    def check(tag):
        copy_batch(cands, [base] * len(cands))
        cands[0].apply(_dops(n, _layer(rng, [k - 1, k])))
        cands[1].apply(_dops(n, _layer(rng, [m - 1, m]) + [("cx", (m - 1, m), ())] + _layer(rng, [m - 1, m])))
        states = cands + [other]
        with split_only():
            got = z_sum_batch(base, states)
        with split_only():
            want = z_all_batch(states).sum(axis=1)
        _report(f"z_sum_batch ({tag}, vs z_all_batch)", cap, float(np.max(np.abs(got - want))))
        np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, err_msg=tag)
        assert cands[0].dims().max() == cap and dims[m] <= cands[1].dims()[m] <= 2 * dims[m + 1]
        return got

    got = check("fresh cache")
    pre = cands[0].preprocessed()
    with W.blas_threads():
        want = sum(M.mps_expectation_z(pre, i) for i in range(n))
    _report("z_sum_batch (one-qubit window at the wide bond, vs oracle)", cap, abs(got[0] - want))
    assert abs(got[0] - want) < ATOL
    assert abs(got[2] - oracle_z(cap).sum()) < ATOL  # the empty window: the prefix state's own sum
    base.apply(_dops(n, _layer(rng, [k])))
    check("prefix changed on a wide-bond site")


@pytest.mark.parametrize("cap", [512, 1024])
def test_pauli_expect_batch_vs_transfer_matrix(cap):
    """Pauli strings whose supports start or end at the two sites beside the widest bond (and the
    full-weight and random strings through it) against the transfer-matrix contraction of the same
    tensors."""
    from adaptaqc_amd.device import pauli_expect_batch

    whichs = (0,) if cap == 1024 else (0, 1)
    states = [loaded(cap, w)[0] for w in whichs]
    n = states[0].n
    labels = W.wide_labels(n, W.widest(W.DIMS[cap]))
    with split_only():
        got = pauli_expect_batch(states, labels)
    assert got.shape == (len(states), len(labels))
    with W.blas_threads():
        want = np.array([[W.mps_pauli_ref(loaded(cap, w)[1], l) for l in labels] for w in whichs])
    _report("pauli_expect_batch", cap, float(np.max(np.abs(got - want))))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    with split_only():
        single = states[-1].pauli_expect(labels)
    np.testing.assert_allclose(got[-1], single, rtol=0, atol=BATCH)


@pytest.mark.parametrize("cap", sorted(W.SAMPLER))
def test_sampler_global_workspace_at_width(cap):
    """130 shots (three shot tiles, the last one short) of the wide state: every shot the
    restatement does not flag as near a boundary equals sampling_ref.mps_sample on the device's own
    tensors, with u passed in and with u drawn on the device."""
    d, _ = loaded(cap)
    n = d.n
    seed, run, shots = W.SAMPLER[cap]
    tensors = d.preprocessed()
    u = ref.uniforms(seed, run, shots, n)
    with W.blas_threads():
        want, near = ref.mps_sample(tensors, u)
    assert near.sum() <= 2
    keep = ~near
    for uu in (u, None):
        with split_only():
            got = d.sample(shots, seed, run, u=uu)
        assert got.dtype == np.uint64 and got.shape == (shots, 1)
        bits = ref.unpack_bits(got, n)
        wrong = int(np.sum(np.any(bits[keep] != want[keep], axis=1)))
        _report("sample (shots that differ)" + ("" if uu is None else " with u passed in"), cap, wrong)
        np.testing.assert_array_equal(bits[keep], want[keep])
        assert not (got[:, -1] >> np.uint64(n)).any()  # no bits past qubit n - 1
    for a, b in zip(d.preprocessed(), tensors):  # the state is not modified
        np.testing.assert_array_equal(a, b)


def test_overlap_amplitudes_and_dot_at_512():
    """<psi|0..0>, every <e_i|psi> and <a|b> of the two capacity-512 states against the oracle's
    contractions (the bars of test_gpu_mps_meas.py and test_gpu_sv_readers.py)."""
    cap = 512
    (a, pre_a), (b, pre_b) = loaded(cap, 0), loaded(cap, 1)
    n = a.n
    with split_only():
        ov = a.overlap_zero()
        amps = a.amps_hw1()
        ab, ba, aa = a.dot(b), b.dot(a), a.dot(a)
    want_ov = M.mps_dot(pre_a, M.zero_mps(n))
    want_amps = np.array([M.extract_amplitude(pre_a, 2 ** i) for i in range(n)])
    with W.blas_threads():
        want_ab = M.mps_dot(pre_a, pre_b)
    _report("overlap_zero", cap, abs(ov - want_ov))
    _report("amps_hw1", cap, float(np.max(np.abs(amps - want_amps))))
    _report("dot", cap, abs(ab - want_ab))
    assert abs(ov - want_ov) < BATCH
    np.testing.assert_allclose(amps, want_amps, rtol=0, atol=BATCH)
    assert abs(want_ab) > 1e-6 and abs(want_ab.imag) > 1e-8  # a wrong conjugation side would show
    assert abs(ab - want_ab) < BATCH
    assert abs(ba - np.conj(want_ab)) < BATCH
    assert abs(aa - 1.0) < BATCH
