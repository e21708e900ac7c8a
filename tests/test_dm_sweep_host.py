"""The host side of the density-matrix engine's Heisenberg-picture pieces: aqc_dm_plan_adjoint's steps
replayed in numpy on a random complex X against the numpy adjoint evolution, unitality, the counts
against the forward plan's, and noise.candidate_superoperator.  No GPU."""
import numpy as np
import pytest

import dm_sweep_ref as sref
import trajectory2_ref as t2ref
from adaptaqc_amd import gates as G
from adaptaqc_amd import noise
from adaptaqc_amd.device import dm_plan

TOL = 1e-10  # the project's FP64 parity tolerance (tests/test_gpu_dm.py)

CASES = [(n, which) for n in (1, 2, 3, 6, 7) for which in "abc"]


@pytest.mark.parametrize("n,which", CASES)
def test_adjoint_plan_replay_matches_the_adjoint_evolution(n, which):
    _, rows, _ = t2ref.program(n, 3, which)
    x = sref.random_matrix(n, 40 + n)
    counts, steps = dm_plan(n, rows, return_steps=True, adjoint=True)
    err = np.max(np.abs(sref.replay_from(n, steps, x) - sref.adjoint(n, rows, x)))
    print(f"n={n} {which}: {counts}, max entry error {err:.3e}")
    assert err <= TOL
    # the identity is a fixed point: every channel is trace preserving
    eye = np.eye(2 ** n, dtype=complex)
    unital = np.max(np.abs(sref.replay_from(n, steps, eye) - eye))
    print(f"  |Lambda^dag(I) - I| = {unital:.3e}")
    assert unital <= TOL
    fwd, fsteps = dm_plan(n, rows, return_steps=True)
    assert counts == fwd and len(steps) == len(fsteps)
    assert np.all(np.diff(steps["segment"]) >= 0) and steps["segment"][-1] == counts["segments"] - 1


@pytest.mark.parametrize("n,which", [(3, "c"), (7, "a")])
def test_adjoint_plan_is_the_forward_plan_backwards(n, which):
    """The forward steps in reverse order, every matrix conjugate-transposed, and the duality
    Tr(X^H Lambda(Y)) = Tr(Lambda^dag(X)^H Y) on the two replays."""
    _, rows, _ = t2ref.program(n, 3, which)
    _, fsteps = dm_plan(n, rows, return_steps=True)
    counts, asteps = dm_plan(n, rows, return_steps=True, adjoint=True)
    for f, a in zip(fsteps[::-1], asteps):
        assert (f["kind"], f["nq"], f["q0"], f["q1"]) == (a["kind"], a["nq"], a["q0"], a["q1"])
        assert f["segment"] + a["segment"] == counts["segments"] - 1
        d = 2 ** int(f["nq"]) if f["kind"] == 0 else 4 ** int(f["nq"])
        fm = np.asarray(f["m"]).view(np.complex128)[: d * d].reshape(d, d)
        am = np.asarray(a["m"]).view(np.complex128)[: d * d].reshape(d, d)
        assert np.array_equal(am, fm.conj().T)
    x, y = sref.random_matrix(n, 1), sref.random_matrix(n, 2)
    lhs = np.vdot(x, sref.replay_from(n, fsteps, y))
    rhs = np.vdot(sref.replay_from(n, asteps, x), y)
    print(f"n={n}: duality gap {abs(lhs - rhs):.3e} of {abs(lhs):.3e}")
    assert abs(lhs - rhs) <= TOL * max(1.0, abs(lhs))


def test_adjoint_plan_argument_errors():
    from adaptaqc_amd._lib import AqcError

    _, rows, _ = t2ref.program(3, 3, "a")
    bad = rows.copy()
    bad["q0"][0] = 3
    with pytest.raises(AqcError, match="aqc_dm_plan_adjoint"):
        dm_plan(3, bad, adjoint=True)
    with pytest.raises(AqcError, match="1 .. 13"):
        dm_plan(14, rows, adjoint=True)
    assert dm_plan(3, rows[:0], adjoint=True)["steps"] == 0


def _lifted(mats):
    """sum_k M_k (x) conj(M_k) at the index r + 2 c, written out entry by entry."""
    s = np.zeros((4, 4), dtype=complex)
    for m in mats:
        for rp in range(2):
            for cp in range(2):
                for r in range(2):
                    for c in range(2):
                        s[rp + 2 * cp, r + 2 * c] += m[rp, r] * np.conj(m[cp, c])
    return s


@pytest.mark.parametrize("name,theta", [("rx", 0.0), ("ry", np.pi / 2), ("rz", -np.pi / 2), ("rx", 0.37)])
def test_candidate_superoperator(name, theta):
    v = G.one_qubit(name, [theta])
    err = noise.thermal_relaxation_error(t2ref.T1, t2ref.T2, 5000)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(err, ["rx", "ry"])
    nm.add_quantum_error(noise.amplitude_damping_error(0.2), "rz", (1,))
    want = _lifted([k @ v for k in err.kraus]) if name != "rz" else _lifted([v])
    assert np.max(np.abs(noise.candidate_superoperator(v, name, 0, nm) - want)) <= 1e-15
    assert np.max(np.abs(noise.candidate_superoperator(v, name, 0, None) - _lifted([v]))) <= 1e-15
    if name == "rz":  # the error attached to qubit 1 only
        damp = noise.amplitude_damping_error(0.2)
        got = noise.candidate_superoperator(v, name, 1, nm)
        assert np.max(np.abs(got - _lifted([k @ v for k in damp.kraus]))) <= 1e-15
    # trace preserving: the rows of the local indices 0 and 3 (r = c) add up to the trace functional
    s = noise.candidate_superoperator(v, name, 0, nm)
    assert np.max(np.abs(s[0] + s[3] - np.array([1, 0, 0, 1]))) <= 1e-12
