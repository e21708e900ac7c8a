"""The fused chain's epilogue inside the Gram SVD (aqc_mps_set_chain_epilogue) against the chain's own
rank and copy phases: the same op lists on the same states with mode 0 and with mode 2, in one
process, leave every Gamma, every lambda, the bond dimensions and the error flags equal bit for bit.

The epilogue decides the rank of an update inside gram_svd_body (svd_gram.h) when the body takes its
narrow path (K <= 64) without a certificate and sigma left S5 sorted, by the rule rank_body runs
(rank_rule, one body for both), and writes the copied site's Gamma from S6's registers instead of
split_copy_body's pass over W.  Every other update -- an unsorted sigma, a declined Gram path, a
certificate, K > 64 -- keeps rank_body and split_copy_body.  aqc_mps_chain_epilogue_stats counts the
updates whose rank the body decided and those it handed back on the sortedness check; with max_chi
<= 64 (K <= 64 on every update) their sum is the Gram path's taken count less its certified ones.

aqc_mps_set_fused_chain(2) sends these batches of 2-3 states through k_chain.  14 qubits at capacity
64 (bonds 1 2 4 8 16 32 64 64 64 32 16 8 4 2 1) is the smallest chain with three neighbouring bonds
at 64: the update on sites (6, 7) is 128 x 128, on (4, 5) 32 x 128 (bonds 16 | 32 | 64: the Gram body
transposes, the copied site is the left one) and on (8, 9) 128 x 32 (the copied site is the right one).
(near_product_mps at this length has bonds 2 3 5 9 17 33 64 33 ...: its update on (6, 7) is 66 x 66, cut
to 64, and its rectangular ones have odd sides.)
"""
import functools

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

N, CAP = 14, 64


@functools.lru_cache(maxsize=None)
def _state(kind, seed, decay=None):
    if kind == "random":
        return bench.random_vidal_mps(N, CAP, seed)
    if kind == "near-product":
        return bench.near_product_mps(N, CAP, seed)
    if kind == "graded":
        return bench.graded_vidal_mps(N, CAP, seed, decay)
    assert kind == "bell"
    # qubits (5, 8) and (6, 7) in Bell pairs, nested, inside a product state: bonds 2 | 4 | 2 around
    # sites 6 and 7, four Schmidt values of 1 / 2 across the bond between them
    rng = np.random.default_rng(seed)
    A = []
    for i in range(N):
        a = rng.uniform(0.1, 0.4)
        A.append(np.array([np.cos(a), np.sin(a)], dtype=complex).reshape(2, 1, 1))
    e = np.eye(2)
    A[5] = e.reshape(2, 1, 2)                                         # [s, 0, a] = d(s, a)
    A[6] = np.einsum("ac,sb->sacb", e, e).reshape(2, 2, 4)            # [s, a, (a', b)] = d(a, a') d(s, b)
    A[7] = np.einsum("ac,sb->sabc", e, e).reshape(2, 4, 2)            # [s, (a, b), a'] = d(s, b) d(a, a')
    A[8] = e.reshape(2, 2, 1)
    return bench.vidal_from_tensors(A)


def _unitary(rng, d):
    q, _ = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    return q


def _run(mode, states, ops_lists, thr, max_chi):
    """The op lists on fresh copies of the states under the epilogue mode: (Aer tuples read back,
    dims, error text or None, epilogue counters, Gram counters)."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS, apply_batch

    L = _lib.lib()
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
        _lib.check(L.aqc_mps_set_chain_epilogue(1))  # (the defaults)
        _lib.check(L.aqc_mps_set_fused_chain(1))
    return out, dims, err, epi, gram


def _both(states, ops_lists, thr=1e-16, max_chi=CAP):
    """Mode 0 and mode 2 on the same inputs, asserted equal bit for bit; mode 2's counters."""
    a_out, a_dims, a_err, a_epi, a_gram = _run(0, states, ops_lists, thr, max_chi)
    b_out, b_dims, b_err, b_epi, b_gram = _run(2, states, ops_lists, thr, max_chi)
    print(f"mode 0: {a_epi} {a_gram} error {a_err}\nmode 2: {b_epi} {b_gram} error {b_err}\n"
          f"dims {[list(map(int, d)) for d in b_dims]}", flush=True)
    assert a_epi == {"fused": 0, "unsorted": 0}, a_epi
    assert a_err == b_err
    assert a_gram == b_gram
    for s, ((ga, la), (gb, lb)) in enumerate(zip(a_out, b_out)):
        assert np.array_equal(a_dims[s], b_dims[s]), (s, a_dims[s], b_dims[s])
        assert len(ga) == len(gb) and len(la) == len(lb)
        for i, (x, y) in enumerate(zip(ga, gb)):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), f"state {s}: Gamma of site {i} differs"
        for i, (x, y) in enumerate(zip(la, lb)):
            assert np.array_equal(x, y), f"state {s}: lambda of bond {i + 1} differs"
    if max_chi and max_chi <= 64:  # K <= 64 on every update: the body's epilogue meets every taken one
        assert b_epi["fused"] + b_epi["unsorted"] == b_gram["taken"] - b_gram["certified"], (b_epi, b_gram)
    return b_epi, b_gram, b_dims, b_err


def _layer(a, b, seed):
    return bench.thin_layer_ops(a, b, np.random.default_rng(seed).uniform(-np.pi, np.pi, 4))


@pytest.mark.parametrize("kind", ["random", "near-product"])
def test_full_update_max_chi_binding(kind):
    """128 x 128 updates cut from 128 to max_chi = 64 (a dense two-qubit gate and a thin layer on
    (6, 7)), and a thin layer on (6, 9): a swap chain of distance 3 out and back."""
    rng = np.random.default_rng(7)
    states = [_state(kind, 1000 + s) for s in range(3)]
    ops = [[(_unitary(rng, 4), (6, 7))], _layer(6, 7, 11), _layer(6, 9, 12)]
    epi, gram, dims, err = _both(states, ops)
    assert err is None
    assert all(int(d[7]) == 64 for d in dims)
    assert epi["fused"] >= 3, epi


def test_rectangular_updates_near_both_ends():
    """Bonds 16 | 32 | 64 (sites 4, 5: theta' 32 x 128, the Gram body's transposed orientation) and
    64 | 32 | 16 (sites 8, 9: 128 x 32): C = 32 < 128, the copied site on either side."""
    rng = np.random.default_rng(8)
    states = [_state("random", 1000), _state("near-product", 1001), _state("random", 1002)]
    ops = [[(_unitary(rng, 4), (4, 5))], [(_unitary(rng, 4), (8, 9))],
           [(_unitary(rng, 4), (4, 5)), (_unitary(rng, 4), (8, 9)), (_unitary(rng, 4), (3, 4)), (_unitary(rng, 4), (9, 10))]]
    epi, gram, dims, err = _both(states, ops)
    assert err is None
    assert epi["fused"] >= 4, epi


def test_tail_rule_cut():
    """Schmidt spectra decaying by 0.9 per value at threshold 1e-8: reduce_zeros' tail rule, not
    max_chi, decides the kept count."""
    states = [_state("graded", 300 + s, 0.9) for s in range(2)]
    ops = [_layer(6, 7, 21), _layer(5, 7, 22)]
    epi, gram, dims, err = _both(states, ops, thr=1e-8)
    assert err is None
    assert all(1 < int(d[7]) < 64 for d in dims), dims
    assert epi["fused"] >= 2, epi


def test_exactly_tied_singular_values():
    """Two nested Bell pairs across the updated bond inside a product state: four Schmidt values of
    1 / 2 that a product of one-qubit unitaries leaves tied.  Whichever way the sortedness check
    goes, the outputs are equal."""
    rng = np.random.default_rng(9)
    states = [_state("bell", 40 + s) for s in range(2)]
    ops = [[(np.kron(_unitary(rng, 2), _unitary(rng, 2)), (6, 7))] for _ in states]
    epi, gram, dims, err = _both(states, ops)
    assert err is None
    assert all(int(d[7]) == 4 for d in dims), dims
    np.testing.assert_allclose(np.concatenate([_state("bell", 40)[1][6]]), 0.5, rtol=0, atol=1e-14)
    assert epi["fused"] + epi["unsorted"] == gram["taken"] - gram["certified"]


def test_gram_path_declined():
    """Spectra decaying by 0.5 per value span more than the Gram path's 1e-9 floor: it declines, the
    register Jacobi and rank_body answer, and the epilogue's counter does not rise."""
    states = [_state("graded", 310 + s, 0.5) for s in range(2)]
    rng = np.random.default_rng(10)
    ops = [[(_unitary(rng, 4), (6, 7))] for _ in states]
    epi, gram, dims, err = _both(states, ops)
    assert err is None
    assert gram["taken"] == 0 and gram["declined_floor"] >= 2, gram
    assert epi == {"fused": 0, "unsorted": 0}, epi


def test_capacity_overflow_flag_arrives():
    """Unbounded max_chi on a 128 x 128 update of full rank: the kept count exceeds the capacity and
    the overflow flag arrives, under either mode."""
    rng = np.random.default_rng(11)
    states = [_state("random", 1000 + s) for s in range(2)]
    ops = [[(_unitary(rng, 4), (6, 7))] for _ in states]
    epi, gram, dims, err = _both(states, ops, max_chi=None)
    assert err is not None and "capacity" in err, err
