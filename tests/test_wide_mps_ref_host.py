"""The wide-bond states and references of wide_mps_ref.py, checked on the host: the bond lists
really fill the split environment chains' column slices the way test_gpu_wide_readers.py relies on
(every workgroup a full slice, some slice above 0 partly filled, some bond that leaves the upper
slices empty), the canonical form keeps those bonds with Schmidt values well above the chop, the
oracle's contractions agree with the dense 2^n vector (the references are right independently of
any device code), and the sampler cases' seeds leave at most 2 shots near a boundary."""
import numpy as np
import pytest

import sampling_ref as ref
import wide_mps_ref as W
from oracle import entanglement as OE

CAPS = sorted(W.DIMS)


def test_slice_table_matches_the_source():
    """SLICES restates env_split_cols / env_split_nw of csrc/ent.hip: read them back from the source
    text, so that a changed split shows here and not as a silently narrower test."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "adaptaqc_amd", "csrc", "ent.hip")).read()
    body = src[src.index("int env_split_cols(int cap)"):]
    cols = {int(c): int(w) for c, w in re.findall(r"case (\d+): return (\d+);", body[:body.index("default:")])}
    m = re.search(r"int env_split_nw\(int cap\) \{ return cap == (\d+) \? (\d+) : kEnvNW; \}", src)
    knw = int(re.search(r"constexpr int kEnvNW = (\d+);", src).group(1))
    for cap, (cw, nw) in W.SLICES.items():
        assert cols[cap] == cw
        assert nw == (int(m.group(2)) if cap == int(m.group(1)) else knw)
        assert cw * nw == cap


@pytest.mark.parametrize("cap", CAPS)
def test_bond_lists_fill_every_slice(cap):
    dims = W.DIMS[cap]
    cw, nw = W.SLICES[cap]
    assert max(dims) == cap
    fill = W.slice_fill(dims, cap)
    assert len(fill) == nw
    for w in range(nw):  # every workgroup has a full slice on some bond
        assert cw in fill[w], w
    partial = [w for w in range(1, nw) if any(0 < c < cw for c in fill[w])]
    assert partial, "no bond ends strictly inside a slice above slice 0"
    # some bond ends below the top slice's first column (cr - c0 < 0 there), and one inside slice 0
    assert any(d < (nw - 1) * cw for d in dims) and any(d < cw for d in dims)
    assert len(fill[nw - 1]) < len(fill[1]) < len(fill[0]) == len(dims)
    k = W.widest(dims)
    assert 3 <= k and k + 3 <= len(dims) - 2  # room for the pairs and labels around the wide bond
    print(f"cap {cap}: n {len(dims) - 1}, widest bond {k}, partly filled slices {partial}")


@pytest.mark.parametrize("cap", CAPS)
def test_states_keep_their_bonds_and_schmidt_floor(cap):
    for which in ((0,) if cap == 1024 else (0, 1)):  # (1024: one state, for the host time)
        aer = W.state(cap, which)
        assert W.bonds_of(aer) == W.DIMS[cap]
        lo = W.min_schmidt(aer)
        print(f"cap {cap} state {which}: smallest Schmidt value {lo:.2e}")
        assert lo >= W.SCHMIDT_FLOOR
        for l in aer[1]:
            assert abs(np.sum(np.asarray(l) ** 2) - 1.0) < 1e-12


@pytest.mark.parametrize("cap", [512, 1024])
def test_left_canonical_state_weighs_every_slice(cap):
    """The left-canonical gauge of the same bond lists: unit norm, identities as left environments,
    and a right environment at the widest bond whose top slice carries its share of the weight
    (within a factor 2 of CW / cap), where the Vidal state's top slice carries less than a
    thousandth of that share (its smallest Schmidt values)."""
    aer = W.flat_state(cap)
    assert W.bonds_of(aer) == W.DIMS[cap]
    pre = W.preprocessed(aer)
    k = W.widest(W.DIMS[cap])
    cw, nw = W.SLICES[cap]
    with W.blas_threads():
        R = ref.right_environments(pre)[k]
        L = np.ones((1, 1), dtype=complex)
        for a in pre[:k]:
            L = sum(a[s].conj().T @ L @ a[s] for s in range(2))
    assert abs(np.trace(R).real - 1.0) < 1e-12
    np.testing.assert_allclose(L, np.eye(cap), rtol=0, atol=1e-12)
    top = float(np.trace(R[-cw:, -cw:]).real)
    lam = np.asarray(W.state(cap)[1][k - 1])
    print(f"cap {cap}: top slice weight {top:.3e} (left-canonical), {np.sum(lam[-cw:] ** 2):.3e} (Vidal)")
    assert cw / cap / 2 < top < 2 * cw / cap
    assert np.sum(lam[-cw:] ** 2) < 1e-3 * cw / cap


def test_ragged_vidal_mps_refuses_unreachable_bonds():
    with pytest.raises(AssertionError):
        W.ragged_vidal_mps([1, 2, 5, 2, 1], 0)  # 5 > 2^2
    with pytest.raises(AssertionError):
        W.ragged_vidal_mps([1, 2, 4, 8, 3, 2, 1], 0)  # 8 > 2 * 3


@pytest.mark.parametrize("cap", [128, 256])
def test_oracle_contractions_agree_with_the_dense_vector(cap):
    """The references against each other: the oracle's <Z> and pair RDMs of the wide state against
    the 2^n vector's, within 1e-13 (n <= 21: capacities 128 and 256)."""
    aer = W.state(cap)
    pre = W.preprocessed(aer)
    n = len(pre)
    psi = W.dense(aer)
    assert abs(np.vdot(psi, psi) - 1.0) < 1e-13
    dz = float(np.max(np.abs(W.oracle_z(pre) - W.dense_z(psi))))
    k = W.widest(W.DIMS[cap])
    pairs = [(0, n - 1), (k - 1, k), (k - 3, k + 2), (k + 3, k - 1)]
    want = np.array([OE.partial_trace_sv(psi, a, b) for a, b in pairs])
    dr = float(np.max(np.abs(W.oracle_rdms(pre, pairs) - want)))
    labels = W.wide_labels(n, k)[:8]
    from sv_readers_ref import sv_pauli_ref

    dp = max(abs(W.mps_pauli_ref(pre, l) - sv_pauli_ref(psi, l)) for l in labels)
    print(f"WIDE_PARITY reference cap {cap}: z {dz:.2e} rdm {dr:.2e} pauli {dp:.2e}")
    assert dz < 1e-13 and dr < 1e-13 and dp < 1e-13


@pytest.mark.parametrize("cap", sorted(W.SAMPLER))
def test_sampler_cases_stay_clear_of_boundaries(cap):
    """The (seed, run, shots) of the device sampler test: on the reference tensors the restatement
    flags at most 2 shots as near a boundary, as test_gpu_sampling.py asks of its cases."""
    seed, run, shots = W.SAMPLER[cap]
    pre = W.preprocessed(W.state(cap))
    with W.blas_threads():
        bits, near = ref.mps_sample(pre, ref.uniforms(seed, run, shots, len(pre)))
    assert shots == 130 and bits.shape == (shots, len(pre))
    assert near.sum() <= 2
    assert 0 < bits.sum() < bits.size
