"""The host side of the noise-aware general gradient on the density-matrix engine: noise.layer_superoperator
against the replayed plan of the same program, noise.terminal_effects against a brute-force adjoint,
gradients.noisy_grads_from_envs on numpy environments against a numpy evolution of every shifted circuit and,
without a noise model, against the reference-structured oracle; aqc_dm_pair_envs's export.  No GPU."""
import ctypes
import functools
import os

import numpy as np
import pytest

import dm_gradient_ref as gref
import dm_ref as dref
import dm_sweep_ref as sref
import trajectory2_ref as t2ref
from adaptaqc_amd import noise
from adaptaqc_amd.device import dm_plan
from adaptaqc_amd.noise import trajectory_program
from conftest import ROOT, to_circuit

TOL = 1e-10  # the project's FP64 parity tolerance (tests/test_gpu_dm.py)


# ---- layer_superoperator ------------------------------------------------------------------------------
def _model2():
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(t2ref.T1, t2ref.T2, 5000), ["rx", "rz"])
    nm.add_quantum_error(noise.amplitude_damping_error(0.2), "ry", (0,))  # on qubit 0 only
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.05, 2), "cx")
    return nm


LAYER2 = [("ry", (0,), (0.4,)), ("ry", (1,), (-0.8,)), ("rx", (1,), (0.3,)), ("cx", (0, 1), ()), ("rz", (0,), (1.1,)),
          ("cx", (1, 0), ()), ("rx", (0,), (-0.6,))]


@pytest.mark.parametrize("qubits", [(0, 1), (1, 0)])
@pytest.mark.parametrize("noisy", [True, False])
def test_layer_superoperator_against_the_replayed_plan(qubits, noisy):
    nm = _model2() if noisy else None
    layer = to_circuit(2, LAYER2)
    got = noise.layer_superoperator(layer, qubits, nm)
    rows, _, _ = trajectory_program(to_circuit(2, gref.placed(LAYER2, *qubits)), nm)
    _, steps = dm_plan(2, rows, return_steps=True)
    want = np.zeros((16, 16), dtype=complex)
    for j in range(16):
        x = np.zeros(16, dtype=complex)
        x[j] = 1.0
        want[:, j] = sref.replay_from(2, steps, x.reshape(4, 4, order="F")).reshape(-1, order="F")
    err = np.max(np.abs(got - want))
    print(f"qubits {qubits}, noisy {noisy}: max entry error {err:.3e}")
    assert err <= TOL
    # dm_ref.replay starts from |00><00|: column 0
    assert np.max(np.abs(got[:, 0].reshape(4, 4, order="F") - dref.replay(2, steps))) <= TOL
    # trace preserving, and (noisy) not unitary
    tr = got[0] + got[5] + got[10] + got[15]
    assert np.max(np.abs(tr - np.eye(4).reshape(-1))) <= 1e-12
    assert (np.max(np.abs(got.conj().T @ got - np.eye(16))) > 1e-3) == noisy


def test_layer_superoperator_tells_the_orientations_apart():
    nm = _model2()
    layer = to_circuit(2, LAYER2)
    a, b = noise.layer_superoperator(layer, (0, 1), nm), noise.layer_superoperator(layer, (1, 0), nm)
    assert np.max(np.abs(a - b)) > 1e-2
    # the same circuit on (3, 1) has no local error on its qubit 0: another map than on (1, 0), equal to the
    # one without the local error
    plain = _model2()
    del plain._local[("ry", (0,))]
    assert np.max(np.abs(noise.layer_superoperator(layer, (3, 1), nm) - noise.layer_superoperator(layer, (1, 0), plain))) <= 1e-15
    with pytest.raises(ValueError):
        noise.layer_superoperator(layer, (1, 1), nm)


# ---- terminal_effects ---------------------------------------------------------------------------------
def _effects_by_adjoint(n, right_ops, nm):
    """|0..0><0..0| pulled back through the whole right-hand program (with its measures) in numpy."""
    rows, _, _ = trajectory_program(gref.with_measures(to_circuit(n, right_ops)), nm)
    x = np.zeros((2 ** n, 2 ** n), dtype=complex)
    x[0, 0] = 1.0
    return sref.adjoint(n, rows, x)


@pytest.mark.parametrize("start", [False, True])
def test_terminal_effects_against_the_adjoint_evolution(start):
    n = 3
    nm = gref.model()
    _, right, _ = gref.case(n, start)
    rhs = gref.with_measures(to_circuit(n, right))
    eff = noise.terminal_effects(n, rhs.data, rhs, nm)
    assert eff.shape == (n, 4)
    want = _effects_by_adjoint(n, right, nm)
    got = dref.kron_all([gref.unpack(e) for e in eff])
    err = np.max(np.abs(got - want))
    print(f"start {start}: max entry error {err:.3e}; effects\n{eff}")
    assert err <= TOL
    assert np.all(eff[:, 2:] == 0) == (not start)  # measure errors alone leave the effects diagonal
    assert np.max(np.abs(eff[:, 1])) > 1e-3  # the relaxation on measure: reading 0 from |1>
    ideal = noise.terminal_effects(n, rhs.data, rhs, None)
    if not start:
        assert np.array_equal(ideal, np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)))


def test_terminal_effects_refuse_an_entangling_right_hand_side():
    rhs = to_circuit(3, [("ry", (0,), (0.3,)), ("cx", (0, 1), ())])
    with pytest.raises(NotImplementedError, match="starting_circuit"):
        noise.terminal_effects(3, rhs.data, rhs, gref.model())


# ---- noisy_grads_from_envs ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(n, start, noisy):
    """(rho in front of the layer, effects, cmap) in numpy."""
    nm = gref.model() if noisy else None
    left, right, _ = gref.case(n, start)
    rows, _, _ = trajectory_program(to_circuit(n, left), nm)
    rho = t2ref.density_matrix(n, rows)
    rhs = gref.with_measures(to_circuit(n, right))
    effects = noise.terminal_effects(n, rhs.data, rhs, nm)
    return rho, effects, gref.full_cmap(n)


@pytest.mark.parametrize("layer,rotoselect", [("THIN", True), ("MIXED", False)])
@pytest.mark.parametrize("start", [False, True])
@pytest.mark.parametrize("n", [3, 4])
def test_noisy_gradients_against_brute_force(n, start, layer, rotoselect):
    from adaptaqc_amd.utils.gradients import noisy_grads_from_envs

    nm = gref.model()
    ops = getattr(gref, layer)
    rho, effects, cmap = _inputs(n, start, True)
    envs = np.stack([gref.pair_env(rho, n, c, t, effects) for c, t in cmap])
    got = np.array(noisy_grads_from_envs(envs, np.trace(rho).real, effects, to_circuit(2, ops), cmap, nm, rotoselect))
    left, right, _ = gref.case(n, start)
    want = np.array(gref.brute_force_gradients(n, left, right, ops, cmap, nm, rotoselect))
    err = np.max(np.abs(got - want))
    print(f"n={n} start={start} {layer}: gradients {want}, max error {err:.3e}")
    assert err <= TOL
    assert want.max() > 1e-2 and np.ptp(want) > 1e-3  # the pairs are told apart
    assert any(c > t for c, t in cmap)


@pytest.mark.parametrize("kind,rotoselect", [("thin", True), ("mixed", False), ("identity_resolvable", True)])
@pytest.mark.parametrize("start", [False, True])
def test_noiseless_gradients_equal_the_reference(kind, rotoselect, start):
    from adaptaqc_amd.utils import ansatzes
    from adaptaqc_amd.utils.gradients import noisy_grads_from_envs
    from oracle import gradients as ogr
    from oracle import mps as M

    n = 4
    rho, effects, cmap = _inputs(n, start, False)
    left, _, start_ops = gref.case(n, start)
    # (the thin layer's own rz generators alone have gradient 0 in front of |0><0| effects: the mixed layer
    # stands for the case without Rotoselect)
    layer = {"thin": lambda: to_circuit(2, gref.THIN), "mixed": lambda: to_circuit(2, gref.MIXED),
             "identity_resolvable": ansatzes.identity_resolvable}[kind]()
    envs = np.stack([gref.pair_env(rho, n, c, t, effects) for c, t in cmap])
    got = np.array(noisy_grads_from_envs(envs, 1.0, effects, layer, cmap, None, rotoselect))
    o_layer = [(i.operation.name, tuple(i.qubits), tuple(i.operation.params)) for i in layer.data]
    o_gens, o_deg = ogr.get_generators_and_degeneracies(o_layer, rotoselect, True)
    psi = M.run_circuit(n, left).preprocessed()
    want = np.array(ogr.general_grad_of_pairs_ref(psi, n, ogr.inverse_ops(o_layer), o_gens, o_deg, cmap, start_ops or ()))
    err = np.max(np.abs(got - want))
    print(f"{kind} rotoselect={rotoselect} start={start}: max error {err:.3e} (gradients up to {want.max():.3f})")
    assert err <= TOL
    assert want.max() > 1e-3  # non-trivial gradients (tests/test_gpu_grad.py's floor)


def test_gradient_argument_errors():
    from adaptaqc_amd.utils.gradients import noisy_grads_from_envs

    rho, effects, cmap = _inputs(3, False, True)
    envs = np.stack([gref.pair_env(rho, 3, c, t, effects) for c, t in cmap])
    bad = to_circuit(2, [("rz", (0,), (0.0,)), ("cz", (0, 1), ())])
    with pytest.raises(ValueError, match="rx, ry, rz and cx"):
        noisy_grads_from_envs(envs, 1.0, effects, bad, cmap, None, True)
    with pytest.raises(ValueError):
        noisy_grads_from_envs(envs[:1], 1.0, effects, to_circuit(2, gref.THIN), cmap, None, True)


# ---- the export ---------------------------------------------------------------------------------------
def test_pair_envs_export_and_signature():
    from adaptaqc_amd import _lib

    assert "aqc_dm_pair_envs" in _lib.EXPORTS
    args, res = _lib._SIGS["aqc_dm_pair_envs"]
    assert list(args) == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert res is ctypes.c_int
    fn = _lib.load().aqc_dm_pair_envs
    assert list(fn.argtypes) == list(args) and fn.restype is ctypes.c_int
    with open(os.path.join(ROOT, "include", "aqc_hip.h")) as f:
        header = " ".join(f.read().split())
    assert ("int aqc_dm_pair_envs(aqc_dm_t h, const int* pairs, int npairs, const double* effects, double* out);"
            in header)
