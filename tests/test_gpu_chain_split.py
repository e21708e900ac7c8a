"""The fused chain's LDS split (chain epilogue 3) against the chain's own phases (mode 0) and the
oracle: the same op lists on the same states under both modes, in one process.

In mode 3 an update that the Gram SVD fuses (narrow path K <= 64, no certificate, sigma sorted) leaves
V and the reciprocals of sigma and of the outer lambdas in the LDS; split_lds_body (mps.hip) writes
the copied site from there and runs the other site's GEMM on all 16 waves over the whole contraction,
three real products per complex one.  The rank decision is mode 1's, so dims, flags, the error text
and the lambda of an update whose inputs are the loaded state are mode 0's bit for bit.  The Gammas
differ from mode 0's in the rounding order of one GEMM and two scalings per update, so the state is
compared as its dense 2^14 vector against the oracle's (oracle.mps.run_circuit on the same ops): both
modes share V, hence the gauge, and with d0 = |psi_mode0 - psi_oracle|, d3 = |psi_mode3 - psi_oracle|
the test requires d3 <= max(2 d0, 64 * 2^-53): a real loss would show as a multiple of d0, and the
floor is the rounding bound of a 128-term dot product.  Updates that mode 3 does not fuse (a declined
Gram path, K > 64) are mode 0's bit for bit.

Shapes as in test_gpu_chain_epilogue.py: 14 qubits at capacity 64 (bonds 1 2 4 8 16 32 64 64 64 32
16 8 4 2 1): 128 x 128 on sites (6, 7), 32 x 128 on (4, 5) and 128 x 32 on (8, 9).

Measured (MI355X; d0, d3 per state): see profiles/chain_split_lds_parity.json.
"""
import functools

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

N, CAP = 14, 64
FLOOR = 64 * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _state(kind, seed, decay=None):
    if kind == "random":
        return bench.random_vidal_mps(N, CAP, seed)
    if kind == "near-product":
        return bench.near_product_mps(N, CAP, seed)
    if kind == "graded":
        return bench.graded_vidal_mps(N, CAP, seed, decay)
    assert kind == "bell"
    # qubits (5, 8) and (6, 7) in nested Bell pairs inside a product state: four Schmidt values of
    # 1 / 2 across the bond between sites 6 and 7
    rng = np.random.default_rng(seed)
    A = []
    for i in range(N):
        a = rng.uniform(0.1, 0.4)
        A.append(np.array([np.cos(a), np.sin(a)], dtype=complex).reshape(2, 1, 1))
    e = np.eye(2)
    A[5] = e.reshape(2, 1, 2)
    A[6] = np.einsum("ac,sb->sacb", e, e).reshape(2, 2, 4)
    A[7] = np.einsum("ac,sb->sabc", e, e).reshape(2, 4, 2)
    A[8] = e.reshape(2, 2, 1)
    return bench.vidal_from_tensors(A)


def _unitary(rng, d):
    q, _ = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    return q


def _layer(a, b, seed):
    return bench.thin_layer_ops(a, b, np.random.default_rng(seed).uniform(-np.pi, np.pi, 4))


def _dense(aer):
    """The 2^N vector of an Aer tuple (qubit 0 the lowest bit of the index)."""
    gam, lam = aer
    v = np.ones((1, 1), dtype=complex)  # [index, bond]
    for i, (g0, g1) in enumerate(gam):
        a = np.stack([g0, g1])
        if i < len(gam) - 1:
            a = a * np.asarray(lam[i])[None, None, :]
        v = np.einsum("xl,slr->sxr", v, a).reshape(-1, a.shape[2])  # the new site is the high bit
    return v[:, 0]


def _oracle(state, ops, thr, max_chi):
    from oracle import mps as M

    o_ops = [("unitary", tuple(q), (np.asarray(m),)) for m, q in ops]
    return _dense(M.run_circuit(N, o_ops, thr, max_chi, mps=M.MPS.from_aer(state)).to_aer())


def _run(mode, states, ops_lists, thr, max_chi):
    """The op lists on fresh copies of the states under the epilogue mode: (Aer tuples read back,
    dims, error text or None, epilogue counters, Gram counters)."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS, apply_batch

    L = _lib.lib()
    before = L.aqc_mps_get_chain_epilogue()
    _lib.check(L.aqc_mps_set_fused_chain(2))
    _lib.check(L.aqc_mps_set_chain_epilogue(mode))
    try:
        work = []
        for q in states:
            d = DeviceMPS(N, CAP, thr, max_chi)
            d.load_aer(q)
            work.append(d)
        _lib.gram_stats()
        _lib.chain_epilogue_stats()
        err = None
        try:
            apply_batch(work, [_lib.ops_array(o) for o in ops_lists], sort=True)
        except _lib.AqcError as e:
            err = str(e)
        epi, gram = _lib.chain_epilogue_stats(), _lib.gram_stats()
        out = [d.to_aer() for d in work]
        dims = [d.dims() for d in work]
        for d in work:
            d.close()
    finally:
        _lib.check(L.aqc_mps_set_chain_epilogue(before))
        _lib.check(L.aqc_mps_set_fused_chain(1))
    return out, dims, err, epi, gram


def _pair(states, ops_lists, thr=1e-16, max_chi=CAP):
    a = _run(0, states, ops_lists, thr, max_chi)
    b = _run(3, states, ops_lists, thr, max_chi)
    print(f"mode 0: {a[3]} {a[4]} error {a[2]}\nmode 3: {b[3]} {b[4]} error {b[2]}\n"
          f"dims {[list(map(int, d)) for d in b[1]]}", flush=True)
    assert a[3] == {"fused": 0, "unsorted": 0}, a[3]
    assert a[2] == b[2]          # the error text (None without one): the flags arrive through it
    assert a[4] == b[4]          # the Gram path's decisions
    for s in range(len(states)):
        assert np.array_equal(a[1][s], b[1][s]), (s, a[1][s], b[1][s])
    return a, b


def _fused_case(name, states, ops_lists, lam_bonds, thr=1e-16, max_chi=CAP, min_fused=1):
    """Both modes, the exact checks, the counters, and the dense states against the oracle.
    lam_bonds[s]: the bonds (index into the Aer lambdas) whose only update takes the loaded state's
    tensors as its inputs, so that its lambda is mode 0's bit for bit."""
    (a_out, a_dims, a_err, a_epi, a_gram), (b_out, b_dims, b_err, b_epi, b_gram) = _pair(states, ops_lists, thr, max_chi)
    assert a_err is None
    assert b_epi["fused"] + b_epi["unsorted"] == b_gram["taken"] - b_gram["certified"], (b_epi, b_gram)
    assert b_epi["fused"] >= min_fused, b_epi
    for s, (st, ops) in enumerate(zip(states, ops_lists)):
        for bond in lam_bonds[s]:
            assert np.array_equal(a_out[s][1][bond], b_out[s][1][bond]), f"state {s}: lambda of bond {bond + 1} differs"
        ref = _oracle(st, ops, thr, max_chi)
        d0 = float(np.linalg.norm(_dense(a_out[s]) - ref))
        d3 = float(np.linalg.norm(_dense(b_out[s]) - ref))
        print(f"parity {name} state {s}: d0 {d0:.3e} d3 {d3:.3e} bound {max(2 * d0, FLOOR):.3e}", flush=True)
        assert d3 <= max(2 * d0, FLOOR), (name, s, d0, d3)
    return b_epi, b_dims


@pytest.mark.parametrize("kind", ["random", "near-product"])
def test_full_update_max_chi_binding(kind):
    """128 x 128 updates cut from 128 to max_chi = 64: a dense two-qubit gate and a thin layer on
    (6, 7), and a thin layer on (6, 9), a swap chain out and back in which the output of one fused
    update is the next one's input."""
    rng = np.random.default_rng(7)
    states = [_state(kind, 1000 + s) for s in range(3)]
    ops = [[(_unitary(rng, 4), (6, 7))], _layer(6, 7, 11), _layer(6, 9, 12)]
    epi, dims = _fused_case(f"full/{kind}", states, ops, [[6], [6], []], min_fused=3)
    assert all(int(d[7]) == 64 for d in dims)


def test_rectangular_updates_both_orientations():
    """Bonds 16 | 32 | 64 (sites 4, 5: theta' 32 x 128, V on the conjugated side, the copied site the
    left one) and 64 | 32 | 16 (sites 8, 9: 128 x 32, the copied site the right one): C = 32 < 128."""
    rng = np.random.default_rng(8)
    states = [_state("random", 1000), _state("near-product", 1001), _state("random", 1002)]
    ops = [[(_unitary(rng, 4), (4, 5))], [(_unitary(rng, 4), (8, 9))],
           [(_unitary(rng, 4), (4, 5)), (_unitary(rng, 4), (8, 9)), (_unitary(rng, 4), (3, 4)), (_unitary(rng, 4), (9, 10))]]
    _fused_case("rectangular", states, ops, [[4], [8], [4, 8]], min_fused=4)


def test_tail_rule_cut_below_64():
    """Schmidt spectra decaying by 0.9 per value at threshold 1e-8: the tail rule decides K < 64."""
    states = [_state("graded", 300 + s, 0.9) for s in range(2)]
    ops = [_layer(6, 7, 21), _layer(5, 7, 22)]
    epi, dims = _fused_case("tail-rule", states, ops, [[6], []], thr=1e-8, min_fused=2)
    assert all(1 < int(d[7]) < 64 for d in dims), dims


def test_exactly_tied_singular_values():
    """Four Schmidt values of 1 / 2 that a product of one-qubit unitaries leaves tied: whichever way
    the sortedness check goes, the state is the oracle's."""
    rng = np.random.default_rng(9)
    states = [_state("bell", 40 + s) for s in range(2)]
    ops = [[(np.kron(_unitary(rng, 2), _unitary(rng, 2)), (6, 7))] for _ in states]
    epi, dims = _fused_case("tied", states, ops, [[], []], min_fused=0)
    assert all(int(d[7]) == 4 for d in dims), dims


def _bitwise(a_out, b_out):
    for s, ((ga, la), (gb, lb)) in enumerate(zip(a_out, b_out)):
        assert len(ga) == len(gb) and len(la) == len(lb)
        for i, (x, y) in enumerate(zip(ga, gb)):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), f"state {s}: Gamma of site {i} differs"
        for i, (x, y) in enumerate(zip(la, lb)):
            assert np.array_equal(x, y), f"state {s}: lambda of bond {i + 1} differs"


def test_declined_gram_path_is_mode_0_bit_for_bit():
    """Spectra decaying by 0.5 per value fall under the Gram path's 1e-9 floor: it declines, the
    register Jacobi, rank_body and the chain's own split answer."""
    states = [_state("graded", 310 + s, 0.5) for s in range(2)]
    rng = np.random.default_rng(10)
    ops = [[(_unitary(rng, 4), (6, 7))] for _ in states]
    (a_out, _, a_err, _, _), (b_out, _, _, b_epi, b_gram) = _pair(states, ops)
    assert a_err is None
    assert b_gram["taken"] == 0 and b_gram["declined_floor"] >= 2, b_gram
    assert b_epi == {"fused": 0, "unsorted": 0}, b_epi
    _bitwise(a_out, b_out)


@pytest.mark.parametrize("thr", [1e-16, 1e-8])
def test_wide_update_is_mode_0_bit_for_bit(thr):
    """max_chi = 128 on a 128 x 128 update of full rank: K > 64, so the update is not fused, whether
    the Gram body declines at its floor (threshold 1e-16: all 128 values are kept) or its tail rule
    cuts a few values first (1e-8): W goes to global memory and the chain's own rank and split run.
    The kept count then exceeds the capacity of 64, with the same text under both modes."""
    rng = np.random.default_rng(12)
    states = [_state("random", 1000 + s) for s in range(2)]
    ops = [[(_unitary(rng, 4), (6, 7))] for _ in states]
    (a_out, _, a_err, _, _), (b_out, _, b_err, b_epi, b_gram) = _pair(states, ops, thr=thr, max_chi=128)
    assert a_err is not None and "capacity" in a_err, a_err   # (more than 64 kept: K > 64)
    assert b_epi == {"fused": 0, "unsorted": 0}, b_epi
    assert b_gram["calls"] >= 2, b_gram
    _bitwise(a_out, b_out)


def test_capacity_overflow_flag_arrives():
    """Unbounded max_chi on a 128 x 128 update of full rank: the kept count exceeds the capacity and
    the overflow flag arrives with the same text under either mode."""
    rng = np.random.default_rng(11)
    states = [_state("random", 1000 + s) for s in range(2)]
    ops = [[(_unitary(rng, 4), (6, 7))] for _ in states]
    (_, _, a_err, _, _), (_, _, b_err, _, _) = _pair(states, ops, max_chi=None)
    assert a_err is not None and "capacity" in a_err and a_err == b_err, (a_err, b_err)
