"""The host side of the density-matrix engine (csrc/dm.hip): aqc_dm_plan's steps replayed in numpy on
vec(rho) against the density-matrix evolution of the trajectory tests, the plan's counts, the argument
errors, and the refusals of DensityMatrixSimulator / DensityMatrixBackend.  No GPU."""
import numpy as np
import pytest

import dm_ref
import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from adaptaqc_amd import _lib
from adaptaqc_amd.device import dm_plan

TOL = 1e-10  # the project's statevector parity tolerance; entries of rho are bounded by 1


def _programs():
    out = [(n, which, 3) for n in (2, 3, 5, 7) for which in "abc"]
    return out


@pytest.mark.parametrize("n,which,depth", _programs())
def test_plan_replay_matches_the_density_matrix(n, which, depth):
    _, rows, _ = t2ref.program(n, depth, which)
    counts, steps = dm_plan(n, rows, return_steps=True)
    got = dm_ref.replay(n, steps)
    want = t2ref.density_matrix(n, rows)
    err = np.max(np.abs(got - want))
    print(f"n={n} {which}: {counts}, max entry error {err:.3e}")
    assert err <= TOL
    assert counts["rows"] == len(rows) and counts["steps"] == len(steps)
    assert counts["tile_bits"] == 2 * min(n, 6) <= 12
    if n <= 6:
        assert counts["segments"] == 1
    # steps come segment by segment
    assert np.all(np.diff(steps["segment"]) >= 0) and steps["segment"][-1] == counts["segments"] - 1


def test_plan_replay_product_errors_and_measure_errors():
    """traj_tomography_ref.program: product errors on cx (two Kraus rows after the gate) and, with a
    terminal measure on every qubit, errors on measure."""
    from adaptaqc_amd.noise import trajectory_program

    qc, rows, _, _ = ttref.program(4, 3)
    for prog in (rows, trajectory_program(_measured(qc), ttref.model())[0]):
        counts, steps = dm_plan(4, prog, return_steps=True)
        err = np.max(np.abs(dm_ref.replay(4, steps) - t2ref.density_matrix(4, prog)))
        print(f"{len(prog)} rows: {counts}, max entry error {err:.3e}")
        assert err <= TOL
        assert counts["segments"] == 1 and counts["rows"] == len(prog)
        # a noisy cx (the gate and the Kraus rows of both qubits) is one step
        assert counts["steps"] < np.count_nonzero(prog["flags"] == 0)
    assert len(prog) > len(rows)  # the measure errors are in the second program


def _measured(qc):
    out = qc.copy()
    for q in range(out.num_qubits):
        out.measure(q, q)
    return out


@pytest.mark.parametrize("n", [7, 12])
def test_fusion_and_tile_size(n):
    _, rows, _ = t2ref.program(n, 8, "a")
    counts, steps = dm_plan(n, rows, return_steps=True)
    print(f"n={n} depth 8: {counts}")
    assert counts["segments"] < counts["steps"] < len(rows)
    assert counts["tile_bits"] <= 12
    assert counts["rows"] == len(rows)
    for s in range(counts["segments"]):  # a segment's qubit set has at most 6 qubits
        mine = steps[steps["segment"] == s]
        qs = set(int(q) for q in mine["q0"]) | set(int(q) for st in mine if st["nq"] == 2 for q in [st["q1"]])
        assert 1 <= len(qs) <= 6
    if n == 7:
        assert np.max(np.abs(dm_ref.replay(n, steps) - t2ref.density_matrix(n, rows))) <= TOL


def test_step_kinds():
    """A noiseless program folds into unitary steps only; a depolarized cx is one 16x16 step."""
    from adaptaqc_amd.noise import trajectory_program
    from conftest import to_circuit

    qc = to_circuit(3, ref.brickwork(3, 2, 5))
    rows, _, _ = trajectory_program(qc, None)
    _, steps = dm_plan(3, rows, return_steps=True)
    assert np.all(steps["kind"] == 0)
    assert np.max(np.abs(dm_ref.replay(3, steps) - t2ref.density_matrix(3, rows))) <= TOL
    _, rows, _ = t2ref.program(2, 1, "a")
    counts, steps = dm_plan(2, rows, return_steps=True)
    assert counts["steps"] == 1 and steps["kind"][0] == 1 and steps["nq"][0] == 2


def _plan_rc(n, rows):
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    counts = np.zeros(4, dtype=np.int32)
    return _lib.load().aqc_dm_plan(int(n), _lib.ptr(rows) if len(rows) else None, len(rows), _lib.ptr(counts), None, 0)


def test_argument_errors():
    _, rows, _ = t2ref.program(3, 1, "a")
    assert _plan_rc(3, rows) == 0
    assert _plan_rc(0, rows[:0]) == -1 and _plan_rc(14, rows[:0]) == -1
    assert _plan_rc(13, rows[:0]) == 0
    group = np.flatnonzero((rows["flags"] & 0xFF) == _lib.OP_KRAUS2)
    missing = np.delete(rows, group[3])  # a group with a missing row
    assert _plan_rc(3, missing) == -1
    assert b"Kraus group" in _lib.load().aqc_last_error()
    bad = rows.copy()
    bad["q0"][0] = 3  # a qubit out of range
    assert _plan_rc(3, bad) == -1
    bad = rows.copy()
    bad["q1"][group[0]: group[0] + 16] = 5
    assert _plan_rc(3, bad) == -1
    meas = rows.copy()
    meas["flags"][0] = _lib.OP_MEASURE1
    assert _plan_rc(3, meas) == -1
    assert b"unknown row flags" in _lib.load().aqc_last_error()
    with pytest.raises(_lib.AqcError):
        dm_plan(3, meas)


def test_simulator_and_backend_refusals():
    from adaptaqc_amd.backends import DensityMatrixBackend, DensityMatrixSimulator, SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from conftest import FakeCompiler

    assert DensityMatrixSimulator.MAX_QUBITS == DensityMatrixBackend.MAX_QUBITS == 13
    wide = QuantumCircuit(14)
    wide.h(0)
    sim = DensityMatrixSimulator(seed=3)
    with pytest.raises(NotImplementedError, match="13 qubits.*trajector"):
        sim.run(wide, shots=16)
    with pytest.raises(NotImplementedError, match="13 qubits.*trajector"):
        sim.pauli_counts(wide, ["I" * 13 + "Z"], shots=16)
    with pytest.raises(ValueError, match="all-identity"):
        sim.pauli_counts(QuantumCircuit(2), ["II"], shots=16)
    be = DensityMatrixBackend()
    with pytest.raises(NotImplementedError, match="13 qubits.*trajector"):
        be.evaluate_global_cost(FakeCompiler(wide))
    small = QuantumCircuit(2)
    small.h(0)
    with pytest.raises(NotImplementedError, match="soften_global_cost"):
        be.evaluate_global_cost(FakeCompiler(small, soften=True))
    general = FakeCompiler(small)
    general.general_initial_state = True
    with pytest.raises(NotImplementedError, match="general_initial_state"):
        be.evaluate_local_cost(general)
    with pytest.raises(ValueError):  # the engine is a simulator of its own, not a method of this one
        SamplingSimulator(method="density_matrix")
