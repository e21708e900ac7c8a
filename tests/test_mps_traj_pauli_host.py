"""Host side of the noisy Pauli readout on the MPS engine (aqc_mps_traj_pauli_counts): its numpy
restatement against the statevector one's, the argument checks of the C entry, and the opt-in keyword
of SamplingSimulator.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import mps_traj_pauli_ref as mpref
import pauli_traj_ref as pref
import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from adaptaqc_amd import _lib, noise


def test_restatement_agrees_with_the_statevector_one():
    """On a 3-qubit program both restatements hold the same states (w = 1), so their values agree to
    rounding, their outcomes wherever neither flags a boundary, and ``plus`` is the column sums."""
    from adaptaqc_amd.paulis import terms_to_codes

    n, shots = 3, 200
    _, rows, n_events, effects = ttref.program(n, 2)
    labels = ["IIX", "IYI", "ZII", "XXI", "ZIY", "XYZ", "ZZZ"]
    codes = terms_to_codes(labels, n)
    u = ref.uniforms(2 ** 40 + 23, 1, shots, n_events + len(labels))
    v, o, plus, near = mpref.pauli_counts(n, rows, codes, effects, u)
    v0, o0, plus0, near0 = pref.pauli_counts(n, rows, codes, effects, u)
    assert v.shape == o.shape == near.shape == (shots, len(labels)) and o.dtype == np.uint8
    assert np.max(np.abs(v - v0)) < 1e-12
    keep = ~(near | near0)
    assert keep.mean() > 0.99
    assert np.array_equal(o[keep], o0[keep])
    assert np.array_equal(plus, np.sum(o == 0, axis=0)) and plus.dtype == np.int64
    if keep.all():
        assert np.array_equal(plus, plus0)


def _call(lib, n, rows, codes, effects, nterms=None, chi_cap=8, shots=4):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    effects = np.ascontiguousarray(effects, dtype=np.float64)
    plus = np.zeros(max(1, len(codes)), dtype=np.int64)
    return lib.aqc_mps_traj_pauli_counts(n, chi_cap, 1e-16, 0, _lib.ptr(rows) if len(rows) else None, len(rows),
                                         _lib.ptr(codes), len(codes) if nterms is None else nterms, _lib.ptr(effects),
                                         shots, ctypes.c_uint64(1), ctypes.c_uint64(0), None, _lib.ptr(plus), None,
                                         None, None)


def test_entry_point_answers_err_arg():
    """Every refusal comes before the first device call (AQC_ERR_ARG = -1)."""
    n = 3
    _, rows, _, effects = ttref.program(n, 1)
    rows = np.ascontiguousarray(rows)
    lib = _lib.load()  # (does not touch the GPU)
    good = np.array([[1, 0, 3]], dtype=np.uint8)
    assert _call(lib, n, rows, [[0, 0, 0]], effects) == -1  # an all-identity term
    assert _call(lib, n, rows, [[1, 4, 0]], effects) == -1  # a code above 3
    assert _call(lib, n, rows, good, effects, nterms=0) == -1
    assert _call(lib, n, rows, good, effects, chi_cap=0) == -1
    assert _call(lib, n, rows, good, effects, chi_cap=1025) == -1
    assert _call(lib, n, rows, good, effects, shots=0) == -1
    assert _call(lib, 0, rows[:0], good, effects) == -1
    _, rows2, _ = t2ref.program(n, 1, "b")  # a correlated (KRAUS2) row
    assert _call(lib, n, np.ascontiguousarray(rows2), good, noise.readout_effects(n, None)) == -1
    bad = np.array(effects, dtype=np.float64)
    bad[1, 2, 0, 0] += 1e-6  # the pair no longer sums to I
    assert _call(lib, n, rows, good, bad) == -1


def test_device_wrapper_refuses_correlated_rows():
    from adaptaqc_amd import device

    _, rows, n_events = t2ref.program(3, 1, "a")
    with pytest.raises(NotImplementedError, match="correlated.*24 qubits"):
        device.mps_trajectory_pauli_counts(3, rows, n_events, ["IIZ"], noise.readout_effects(3, None), 4, 1)


def test_simulator_keyword():
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator

    with pytest.raises(ValueError, match="mps_trajectories"):
        SamplingSimulator(mps_pauli_readout=True)
    with pytest.raises(ValueError, match="mps_trajectories"):
        SamplingSimulator(method="matrix_product_state", mps_pauli_readout=True)
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, mps_pauli_readout=True)
    assert sim.mps_pauli_readout and sim.mps_trajectories
    assert not SamplingSimulator(mps_trajectories=True).mps_pauli_readout
    # a correlated model is refused before anything runs
    qc, _, _ = t2ref.program(3, 1, "a")
    with pytest.raises(NotImplementedError, match="correlated.*24 qubits"):
        sim.pauli_counts(qc, ["IIZ"], shots=10, noise_model=t2ref.model("a"))
    assert sim.runs == 0
    # without the keyword the earlier refusal stands, now saying how to opt in
    plain = SamplingSimulator(method="matrix_product_state", mps_trajectories=True)
    with pytest.raises(NotImplementedError, match="Pauli readout of MPS trajectories is not built.*mps_pauli_readout=True"):
        plain.pauli_counts(qc, ["IIZ"], shots=10, noise_model=ttref.model())
    assert plain.runs == 0


def test_symbol_is_exported_and_declared():
    """The header / EXPORTS comparison of test_capi holds with the new symbol in both."""
    import os
    import re

    assert "aqc_mps_traj_pauli_counts" in _lib.EXPORTS
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "aqc_hip.h")
    with open(header) as f:
        assert re.search(r"^int aqc_mps_traj_pauli_counts\(", f.read(), re.M)
    assert hasattr(_lib.load(), "aqc_mps_traj_pauli_counts")
