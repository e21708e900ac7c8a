"""The statevector readers on MI355X (z_all, pair_rdms, transition, pauli_expect, sample) against
the numpy references of sv_readers_ref.py, at the sizes where their reductions span more than one
workgroup, chunk or tile, and DeviceMPS.dot against oracle.mps.mps_dot as a complex number.

States are loaded with DeviceSV.set unless a test says otherwise, and every reader is followed by a
check that the state it read is bit for bit what was set.

Tolerances: 1e-12 on z, RDMs and transition matrices of normalised states (the statevector bar of
test_gpu_sv.py: a tree reduction of 2^20 terms summing to O(1) carries about 20 eps, the serial pass
over at most 1024 partials at most 1024 eps = 2e-13); 1e-11 on Pauli terms (test_gpu_pauli.py)."""
import numpy as np
import pytest

import sampling_ref
import sv_readers_ref as R
from conftest import to_circuit
from oracle import mps as M
from oracle import sv as osv
from oracle.entanglement import partial_trace_sv

pytestmark = pytest.mark.gpu

ATOL = 1e-12
PAULI_ATOL = 1e-11

_DENSE = {}


def dense(n, seed_base=1000):
    """(device state, psi) with psi = random_state(n, seed_base + n) set once; tests do not modify them."""
    from adaptaqc_amd.device import DeviceSV

    if (n, seed_base) not in _DENSE:
        psi = R.random_state(n, seed_base + n)
        d = DeviceSV(n)
        d.set(psi)
        _DENSE[(n, seed_base)] = (d, psi)
    return _DENSE[(n, seed_base)]


def device_of(psi):
    from adaptaqc_amd.device import DeviceSV

    d = DeviceSV(int(round(np.log2(len(psi)))))
    d.set(psi)
    return d


def unchanged(d, psi):
    np.testing.assert_array_equal(d.get(), psi)  # the readers do not modify the state


# ---- 3.1 z_all ---------------------------------------------------------------------------------
# k_sv_zpartial: bits 0-7 from the thread id, 8-11 from the per-thread chunk, >= 12 from the block
# index; n <= 12 is one block (x < dim guards n < 12), n = 13, 14, 15 are 2, 4, 8 blocks.
@pytest.mark.parametrize("n", range(1, 16))
def test_z_all(n):
    d, psi = dense(n)
    np.testing.assert_allclose(d.z_all(), R.z_ref(psi, n), rtol=0, atol=ATOL)
    unchanged(d, psi)
    last = R.basis_state(n, 2 ** n - 1)
    e = device_of(last)
    assert np.array_equal(e.z_all(), -np.ones(n))  # exactly
    unchanged(e, last)
    first = R.basis_state(n, 0)
    e.set(first)
    assert np.array_equal(e.z_all(), np.ones(n))  # exactly
    unchanged(e, first)


# ---- 3.2 pair_rdms -----------------------------------------------------------------------------
def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def check_rdms(n, pairs):
    d, psi = dense(n)
    refs = {}
    for a, b in pairs:
        key = (min(a, b), max(a, b))
        if key not in refs:
            refs[key] = partial_trace_sv(psi, a, b)
    got = d.pair_rdms(pairs)
    assert got.shape == (len(pairs), 4, 4)
    want = np.array([refs[(min(a, b), max(a, b))] for a, b in pairs])
    print("rdm n", n, "pairs", len(pairs), "max abs err", np.max(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    np.testing.assert_allclose(got, np.conj(np.transpose(got, (0, 2, 1))), rtol=0, atol=ATOL)  # Hermitian
    np.testing.assert_allclose(np.trace(got, axis1=1, axis2=2), 1.0, rtol=0, atol=ATOL)
    np.testing.assert_allclose(d.pair_rdms([(b, a) for a, b in pairs]), got, rtol=0, atol=ATOL)
    unchanged(d, psi)


# chunks = max(1, min(2^(n-2) / 1024, ceil(2048 / npairs))) workgroups a pair
RDM_CASES = {
    "n2": (2, [(0, 1), (1, 0)]),  # rest = 1: 1 chunk, one thread with work
    "n3": (3, all_pairs(3)),  # rest = 2, 1 chunk
    "n12_all": (12, all_pairs(12)),  # rest = 1024: the last size with 1 chunk
    "n13_all": (13, all_pairs(13)),  # rest = 2048: the first size with 2 chunks
    "n16_all": (16, all_pairs(16)),  # 120 pairs: min(16, 18) = 16 chunks
    "n16_one_pair": (16, [(0, 15)]),  # min(16, 2048) = 16 chunks, grid y = 1
    "n16_1500": (16, [all_pairs(16)[i % 120] for i in range(1500)]),  # min(16, 2) = 2 chunks
    "n16_2100": (16, [all_pairs(16)[i % 120] for i in range(2100)]),  # 1 chunk, 64 grid-stride steps
    "n20": (20, [(0, 1), (0, 19), (18, 19), (3, 12), (12, 3), (11, 12)]),  # min(256, 342) = 256 chunks
}


@pytest.mark.parametrize("case", list(RDM_CASES))
def test_pair_rdms(case):
    n, pairs = RDM_CASES[case]
    check_rdms(n, pairs)


def test_pair_rdms_refusals():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import DeviceSV

    one = DeviceSV(1)
    with pytest.raises(AqcError, match="-1"):
        one.pair_rdms([(0, 1)])
    with pytest.raises(AqcError, match="-1"):
        one.pair_rdms([(0, 0)])
    d, psi = dense(3)
    for bad in ((1, 1), (0, 3), (3, 0), (-1, 2)):
        with pytest.raises(AqcError, match="-1"):
            d.pair_rdms([(0, 1), bad])
    unchanged(d, psi)


# ---- 3.3 transition ----------------------------------------------------------------------------
# chunks = max(1, min(1024, 2^(n-1) / 1024)): 1 up to n = 11, 2 at n = 12, 32 at n = 16, 512 at n = 20
TRANSITION_CASES = [(n, q) for n in (1, 2, 11, 12) for q in range(n)] + [(16, 0), (16, 7), (16, 15), (20, 0), (20, 19)]


@pytest.mark.parametrize("n,q", TRANSITION_CASES)
def test_transition_of_two_dense_states(n, q):
    (bra, bra_psi), (ket, ket_psi) = dense(n), dense(n, 2000)
    got = bra.transition(ket, q)
    want = R.transition_ref(bra_psi, ket_psi, n, q)
    print("transition n", n, "q", q, "max abs err", np.max(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    unchanged(bra, bra_psi)
    unchanged(ket, ket_psi)


@pytest.mark.parametrize("n", [12, 16])  # 2 and 32 chunks
def test_transition_identities(n):
    from adaptaqc_amd.device import DeviceSV

    (bra, bra_psi), (ket, ket_psi) = dense(n), dense(n, 2000)
    work = DeviceSV(n)
    for q in (0, n // 2, n - 1):
        # bra is ket: the transposed one-qubit RDM
        same = bra.transition(bra, q)
        m = bra_psi.reshape(2 ** (n - 1 - q), 2, 2 ** q)
        np.testing.assert_allclose(same, np.einsum("hal,hbl->ab", m, m.conj()).T, rtol=0, atol=ATOL)
        assert abs(np.trace(same) - 1.0) < ATOL
        # swapping bra and ket: the conjugate transpose
        t = bra.transition(ket, q)
        np.testing.assert_allclose(ket.transition(bra, q), t.conj().T, rtol=0, atol=ATOL)
        # sum_ab V[a][b] T[a][b] = <bra| V_q |ket>, with V applied to ket by the device
        v = R.random_unitary(100 * n + q)
        work.set(ket_psi)
        work.apply([(v, (q,))])
        assert abs(np.sum(v * t) - np.vdot(bra_psi, work.get())) < ATOL
        assert abs(np.sum(v * t) - np.vdot(bra_psi, R.apply_1q(ket_psi, n, q, v))) < ATOL
    unchanged(bra, bra_psi)
    unchanged(ket, ket_psi)


def test_transition_refusals():
    from adaptaqc_amd._lib import AqcError

    (a, a_psi), (b, _) = dense(3), dense(2)
    with pytest.raises(AqcError, match="-1"):
        a.transition(b, 0)
    for q in (-1, 3):
        with pytest.raises(AqcError, match="-1"):
            a.transition(a, q)
    unchanged(a, a_psi)


# ---- 3.4 pauli_expect --------------------------------------------------------------------------
def single(n, q, p):
    chars = ["I"] * n
    chars[n - 1 - q] = p
    return "".join(chars)


def pauli_labels(n):
    """All-identity, X / Y / Z alone on qubits 0, 12, 13 and n - 1 (those below n), the full-weight
    string, XX...X (k ^ x reaches the far end of the array) and 20 seeded random strings."""
    rng = np.random.default_rng(7000 + n)
    out = ["I" * n]
    out += [single(n, q, p) for q in sorted({0, 12, 13, n - 1}) if q < n for p in "XYZ"]
    out += ["".join(rng.choice(list("XYZ"), n)), "X" * n]
    out += ["".join(rng.choice(list("IXYZ"), n)) for _ in range(20)]
    return out


def pauli_labels_21():
    rng = np.random.default_rng(7021)
    return ["I" * 21, single(21, 20, "Y"), single(21, 0, "X"), "X" * 21, "".join(rng.choice(list("XYZ"), 21)),
            "".join(rng.choice(list("IXYZ"), 21))]


# blocks a term = min(256, max(1, 2^n / 4096)): 1, 16, 256 (the cap), and 256 with two grid-stride
# steps a thread at n = 21
@pytest.mark.parametrize("n", [12, 16, 20, 21])
def test_pauli_expect(n):
    d, psi = dense(n)
    labels = pauli_labels_21() if n == 21 else pauli_labels(n)
    got = d.pauli_expect(labels)
    want = np.array([R.sv_pauli_ref(psi, l) for l in labels])
    print("pauli n", n, "terms", len(labels), "max abs err", np.max(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=PAULI_ATOL)
    assert abs(got[0] - np.vdot(psi, psi).real) < PAULI_ATOL  # the all-identity term
    assert np.array_equal(d.pauli_expect(labels), got)  # bit-identical: fixed order, no atomics
    unchanged(d, psi)


# ---- 3.5 sample --------------------------------------------------------------------------------
def check_shots(got, want, near, neighbours):
    assert got.dtype == np.uint64 and got.shape == want.shape
    got = got.astype(np.int64)
    for j in np.flatnonzero(got != want):
        assert near[j] and got[j] in neighbours(want[j]), (j, got[j], want[j])


# tiles of 4096 amplitudes: 1, 4, 16, 256 for the dense cases; 16 for the sparse ones at n = 16;
# 8192 at n = 25 (two chunks of the tile scan, 13 steps of the binary search)
@pytest.mark.parametrize("name", [c["name"] for c in R.SAMPLING_CASES])
def test_sample_matches_inverse_cdf(name):
    from adaptaqc_amd.device import DeviceSV

    case, idx, amps, u, want, near = R.sampling_case(name)
    n, shots = case["n"], case["shots"]
    assert near.sum() <= 2
    if case["dense"]:
        d, psi = dense(n)
        np.testing.assert_array_equal(psi, amps)
    else:
        psi = R.embed(n, idx, amps)
        d = DeviceSV(n)
        d.set(psi)
    for got in (d.sample(shots, R.SEED + n, R.RUN, u=u), d.sample(shots, R.SEED + n, R.RUN)):
        check_shots(got, want, near, lambda k: R.sparse_neighbours(idx, amps, k))
    if n < 25:  # (the 2^25 state is only sampled, never read back)
        unchanged(d, psi)


def test_sample_exact_ties_on_the_uniform_state():
    """Every amplitude 2^-8 at n = 16: probabilities, tile sums and prefix sums are exact in double,
    so u = k / 2^16 sits on a boundary exactly and the outcome is k, with no near allowance.
    k = 4096 is the first amplitude of tile 1 (residual 0), 4095 the last of tile 0."""
    n = 16
    psi = np.full(2 ** n, 2.0 ** -8, dtype=complex)
    d = device_of(psi)
    ks = np.array([0, 1, 4095, 4096, 4097, 65535])
    u = np.concatenate([ks / 2.0 ** 16, [0.0, 1.0 - 2.0 ** -53]])
    got = d.sample(len(u), 1, u=u)
    assert list(got) == list(ks) + [0, 65535]
    unchanged(d, psi)


def test_sample_edge_u_on_a_sparse_state():
    """Weight in tiles 1 and 14 only: u = 0 skips the empty tile 0 to the first supported index,
    u = 1 - 2^-53 gives the last one (tile 15 is empty)."""
    idx, amps = R.tiles_1_and_14()
    psi = R.embed(16, idx, amps)
    d = device_of(psi)
    got = d.sample(2, 1, u=np.array([0.0, 1.0 - 2.0 ** -53]))
    assert list(got) == [idx.min(), idx.max()]
    unchanged(d, psi)


def test_sample_of_the_zero_vector():
    psi = np.zeros(2 ** 14, dtype=complex)
    d = device_of(psi)
    assert not d.sample(300, 5).any()  # the documented behaviour of k_sv_shots: outcome 0
    unchanged(d, psi)


# ---- 3.6 readers straight after a register-tile apply ------------------------------------------
def test_readers_after_register_tile_apply():
    """n = 14 is the first size on the register-tile path.  Both states are left by apply with no
    read in between; transition comes first, while the bra's passes are still queued on its stream."""
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceSV

    n = 14
    ops_a = sampling_ref.brickwork(n, 4, 5) + [("cx", (13, 0), ())]
    ops_b = sampling_ref.brickwork(n, 3, 6)
    dev_a, dev_b = device_ops(to_circuit(n, ops_a)), device_ops(to_circuit(n, ops_b))
    psi_a, psi_b = osv.simulate(n, ops_a), osv.simulate(n, ops_b)
    a, b = DeviceSV(n), DeviceSV(n)
    a.apply(dev_a)
    b.apply(dev_b)
    t = a.transition(b, 5)  # 8 chunks
    np.testing.assert_allclose(t, R.transition_ref(psi_a, psi_b, n, 5), rtol=0, atol=ATOL)
    np.testing.assert_allclose(a.z_all(), R.z_ref(psi_a, n), rtol=0, atol=ATOL)  # 4 blocks
    pairs = [(0, 13), (6, 7)]  # 4 chunks each
    want = np.array([partial_trace_sv(psi_a, p, q) for p, q in pairs])
    np.testing.assert_allclose(a.pair_rdms(pairs), want, rtol=0, atol=ATOL)
    rng = np.random.default_rng(14)
    labels = ["I" * n, single(n, 13, "Y"), "X" * n] + ["".join(rng.choice(list("IXYZ"), n)) for _ in range(2)]
    got = a.pauli_expect(labels)  # 4 blocks a term
    np.testing.assert_allclose(got, [R.sv_pauli_ref(psi_a, l) for l in labels], rtol=0, atol=ATOL)
    shots = 200
    u = R.philox_u(n, shots)
    want, near = sampling_ref.sv_sample(psi_a, u)  # 4 tiles
    assert near.sum() <= 2
    check_shots(a.sample(shots, R.SEED + n, R.RUN), want, near, lambda k: sampling_ref.sv_neighbours(psi_a, k))
    np.testing.assert_allclose(a.get(), psi_a, rtol=0, atol=ATOL)
    np.testing.assert_allclose(b.get(), psi_b, rtol=0, atol=ATOL)


# ---- 3.7 DeviceMPS.dot -------------------------------------------------------------------------
def _loaded(n, chi, cap, seed):
    import bench
    from adaptaqc_amd.device import DeviceMPS

    aer = bench.random_vidal_mps(n, chi, seed)
    d = DeviceMPS(n, cap)
    d.load_aer(aer)
    return d, aer


@pytest.mark.parametrize("n,chi_a,chi_b,cap", [(12, 8, 32, 32), (14, 48, 96, 128)])
def test_mps_dot_is_a_complex_inner_product(n, chi_a, chi_b, cap):
    """<a|b> with a conjugated, for two states of different bond dimensions in one capacity."""
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS

    a, aer_a = _loaded(n, chi_a, cap, 300 + n)
    b, aer_b = _loaded(n, chi_b, cap, 400 + n)
    assert a.dims().max() == chi_a and b.dims().max() == chi_b
    pre_a, pre_b = M.MPS.from_aer(aer_a).preprocessed(), M.MPS.from_aer(aer_b).preprocessed()
    want = M.mps_dot(pre_a, pre_b)
    assert abs(want.imag) > 1e-4 and abs(want.real) > 1e-4  # a wrong conjugation side would show
    got = a.dot(b)
    print("mps dot n", n, "err", abs(got - want))
    assert abs(got - want) < 1e-12
    assert abs(b.dot(a) - np.conj(want)) < 1e-12
    for d in (a, b):
        self_dot = d.dot(d)
        assert abs(self_dot - 1.0) < 1e-12 and abs(self_dot.imag) < 1e-14
    # a long-range gate leaves the qubits out of site order: dot has to sort first
    gate = [("cx", (2, n - 5), ())]
    a.apply(device_ops(to_circuit(n, gate)))
    # the contraction alone: against the tensors of a copy taken before dot sorts a (the copy keeps
    # the site order, and reading it back sorts the copy by the same deterministic updates)
    c = DeviceMPS(n, cap)
    c.copy_from(a)
    got_g = a.dot(b)
    want_g = M.mps_dot(c.preprocessed(), pre_b)
    assert abs(want_g - want) > 1e-3
    print("mps dot after cx, n", n, "err", abs(got_g - want_g))
    assert abs(got_g - want_g) < 1e-12
    assert abs(b.dot(a) - np.conj(want_g)) < 1e-12
    # and the gate with it, against the oracle's replay (1e-10: the bar on overlaps of test_gpu_sv.py)
    pre_g = M.run_circuit(n, gate, 1e-16, None, mps=M.MPS.from_aer(aer_a)).preprocessed()
    print("mps dot after cx vs oracle replay, n", n, "err", abs(got_g - M.mps_dot(pre_g, pre_b)))
    assert abs(got_g - M.mps_dot(pre_g, pre_b)) < 1e-10
    # refusals: another capacity, another n
    with pytest.raises(AqcError, match="-1"):
        a.dot(DeviceMPS(n, 2 * cap))
    with pytest.raises(AqcError, match="-1"):
        a.dot(DeviceMPS(n - 1, cap))
